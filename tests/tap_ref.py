"""Reference of the channel taps: the rule of include/zfft.h (zfft_plan_taps) in numpy float64,
written straight from the formula with an exact integer phase -- never a call into the library.

    y[m] = sum_{k<T} h[k] x[m D - k] exp(-2 pi i ((fw (m D - k)) mod 2^32) / 2^32),  m D >= n_open

x is whatever the plan's in_dtype loader makes of the caller's samples in float32 (`loader`), 0
before the start of the count.  The error gate is derived, not measured (`gate`): T rounded
products in a fixed-order float32 sum, the table's rounding, and the rotation's phase, sincos and
complex multiply bound |y - y_ref| by (T + 32) 2^-24 sum|h| max|x|.

Below that, rule 7 in float32 (tap_f32 on tests/f32_exact.py), rounded where the header says the
kernel rounds, for the comparisons that are equalities (tests/test_gpu_tap_exact.py)."""
import numpy as np

TWO32 = 1 << 32
DT_TAPS = [(1, 1), (2, 3), (3, 25), (8, 65), (32, 257), (200, 1601)]


def ceil_div(a, d):
    return -(-int(a) // int(d))


def count(n0, n_open, n, D):
    """Outputs of a push of n samples at count n0 for a tap opened at n_open."""
    return max(0, ceil_div(n0 + n, D) - ceil_div(max(n0, n_open), D))


def outputs(n0, n_open, n, D):
    """The m of those outputs."""
    return np.arange(ceil_div(max(n0, n_open), D), max(ceil_div(n0 + n, D), ceil_div(max(n0, n_open), D)),
                     dtype=np.int64)


def loader(x, in_dtype):
    """The samples as the loader defines them: float32 values, returned as complex128."""
    x = np.asarray(x)
    if in_dtype == "complex64":
        return x.astype(np.complex64).astype(np.complex128)
    if in_dtype == "complex32":   # interleaved float16 I, Q
        v = x.astype(np.float16).astype(np.float32).reshape(-1, 2)
    elif in_dtype == "cu8":       # RTL-SDR bytes: (b - 127.5) * (1 / 127.5) in float32
        v = ((x.astype(np.float32) - np.float32(127.5)) * np.float32(1.0 / 127.5)).reshape(-1, 2)
    elif in_dtype == "f32":
        return x.astype(np.float32).astype(np.float64) + 0j
    else:
        raise ValueError(in_dtype)
    return v[:, 0].astype(np.float64) + 1j * v[:, 1].astype(np.float64)


def ref_tap(x, n_first, fw, D, h, ms, block=1 << 21):
    """y[m], m in ms, for the stream whose sample n_first + i is x[i] and every other sample 0."""
    x = np.asarray(x, dtype=np.complex128)
    h = np.asarray(h, dtype=np.float64)
    ms = np.asarray(ms, dtype=np.int64)
    T = h.size
    k = np.arange(T, dtype=np.int64)
    out = np.zeros(ms.size, dtype=np.complex128)
    step = max(1, block // T)
    fwu = np.uint64(int(fw) % TWO32)
    for a in range(0, ms.size, step):
        idx = ms[a:a + step, None] * np.int64(D) - k[None, :]
        rel = idx - np.int64(n_first)
        ok = (rel >= 0) & (rel < x.size)
        xv = np.where(ok, x[np.clip(rel, 0, max(x.size - 1, 0))], 0.0)
        ph = (fwu * (idx % TWO32).astype(np.uint64)) % np.uint64(TWO32)   # exact: both factors < 2^32
        rot = np.exp(-2j * np.pi * (ph.astype(np.float64) / TWO32))
        out[a:a + step] = (h[None, :] * xv * rot).sum(axis=1)
    return out


def ref_push(x, n0, fw, D, h, n_open=None):
    """All outputs of one push of x at count n0 (the past all zero)."""
    return ref_tap(x, n0, fw, D, h, outputs(n0, n0 if n_open is None else n_open, len(x), D))


def gate(h, xmax):
    h = np.asarray(h, dtype=np.float64)
    return (h.size + 32) * 2.0 ** -24 * np.abs(h).sum() * float(xmax)


def freq_word(f_hz, fs):
    return (int(round(float(f_hz) / fs * 2.0 ** 32)) + 2 ** 31) % TWO32 - 2 ** 31


def solid_taps(T, seed):
    """Caller-supplied taps with no small entries: |h[k]| in [0.5, 1], random signs."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.5, 1.0, T) * rng.choice([-1.0, 1.0], T)).astype(np.float32)


def noise_and_tones(n, seed, fs=1.0, tones=((0.013, 0.5), (-0.21, 0.25))):
    """complex64 noise plus tones (cycles per sample, amplitude), |x| below about 1.3."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    x = 0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for f, a in tones:
        x += a * np.exp(2j * np.pi * f * t)
    return x.astype(np.complex64)


# ---------------------------------------------------------------- the rule in float32, bit for bit
def quarter_word(D):
    """A freq_word with (fw D) mod 2^30 == 0, so that rot(m) is always a whole quarter turn, and a
    fully complex table: 5 2^30 / gcd(D, 2^30), or None where D leaves only the multiples
    of 2^30 (whose table is real or imaginary)."""
    p = 1
    while D % (2 * p) == 0:
        p *= 2
    return None if p == 1 else ((5 << 30) // p + (1 << 31)) % TWO32 - (1 << 31)


def tap_f32(x, n_first, fw, D, c, ms, block=1 << 15):
    """Rule 7 in float32 (tests/f32_exact.py), bit for bit: y[m], m in ms, for the stream whose sample
    n_first + i is the loader's float32 value x[i] (complex64) and every other sample 0, with the
    table c = zfft_tap_table(fw, h).  Four partial sums a_j over the k = j (mod 4) in ascending k from
    +0, each step two fmas per component in the header's order (re: fma(c.re, x.re, a.re), then
    fma(-c.im, x.im, .); im: fma(c.re, x.im, a.im), then fma(c.im, x.re, .)), joined as (a_0 + a_1) +
    (a_2 + a_3); then the rotation rot(m) = exp(-2 pi i ((fw m D) mod 2^32) / 2^32), restricted to
    (fw D) mod 2^30 == 0, where it is exactly 1, -i, -1 or i and the product a swap and a sign."""
    import f32_exact as fx
    assert (int(fw) * int(D)) % (1 << 30) == 0, (fw, D)
    x = np.ascontiguousarray(x, dtype=np.complex64)
    c = np.ascontiguousarray(c, dtype=np.complex64)
    T = c.size
    c_re, c_im = np.ascontiguousarray(c.real), np.ascontiguousarray(c.imag)
    xp = np.concatenate([np.zeros(T - 1, np.complex64), x])
    x_re, x_im = np.ascontiguousarray(xp.real), np.ascontiguousarray(xp.imag)
    at = np.array([int(m) * int(D) - int(n_first) + T - 1 for m in ms], dtype=np.int64)
    assert at.size == 0 or (at.min() >= T - 1 and at.max() < xp.size)
    out = np.zeros(at.size, np.complex64)
    for b in range(0, at.size, block):
        i = at[b:b + block]
        re = [np.zeros(i.size, np.float32) for _ in range(4)]
        im = [np.zeros(i.size, np.float32) for _ in range(4)]
        for k in range(T):
            j, vr, vi = k & 3, x_re[i - k], x_im[i - k]
            re[j] = fx.fma(-c_im[k], vi, fx.fma(c_re[k], vr, re[j]))
            im[j] = fx.fma(c_im[k], vr, fx.fma(c_re[k], vi, im[j]))
        y_re = fx.add(fx.add(re[0], re[1]), fx.add(re[2], re[3]))
        y_im = fx.add(fx.add(im[0], im[1]), fx.add(im[2], im[3]))
        q = np.array([((((int(fw) % TWO32) * ((int(m) * int(D)) % TWO32)) % TWO32) >> 30) for m in ms[b:b + block]])
        out[b:b + block].real = np.choose(q, [y_re, y_im, -y_re, -y_im])      # rot = 1, -i, -1, i
        out[b:b + block].imag = np.choose(q, [y_im, -y_re, -y_im, y_re])
    return out


def model_push(x, n0, fw, D, c, n_open=None):
    """All outputs of one push of x at count n0 (the past all zero), in float32."""
    return tap_f32(x, n0, fw, D, c, outputs(n0, n0 if n_open is None else n_open, len(x), D))
