"""Reference of the demodulator bank: the rule of include/zfft.h (zfft_plan_demod) in numpy
float64, written straight from the formulas with an exact integer phase -- never a call into the
library.

    a[m, s] = sum_{k<Ta} g[k] d_s[m Da - k],   m Da >= the start,
    d = |x| (AM), arg(x[n] conj(x[n-1])) / pi (FM, 0 where the product is 0),
        Re(x[n] exp(+2 pi i ((w n) mod 2^32) / 2^32)) (SSB), |x|^2 (POWER),

x the streams' complex64 values, 0 before the start of the count.  The error gate is the header's
rule 6 (`gate`): (Ta + 32) 2^-24 sum|g| max|d| for the filter and sum|g| eps_mode for the detector,
eps derived for AM, SSB and POWER and, for FM, EPS_FM 2^-24 -- twice the worst detector error the
first run on the device measured (profiles/demod/README.md), under the condition EPS_FM <= 16.

Below that, the same rule in float32 (detect_f32, fir_f32 on tests/f32_exact.py): every product,
fused multiply-add, square root and sum rounded where the header says the kernel rounds, for the
comparisons that are equalities (tests/test_gpu_demod_exact.py, test_gpu_demod_edges.py)."""
import numpy as np

TWO32 = 1 << 32
U = 2.0 ** -24
AM, FM, SSB, POWER = 0, 1, 2, 3
MODES = {"am": AM, "fm": FM, "ssb": SSB, "power": POWER}
EPS_FM = 3             # ZFFT_DEMOD_EPS_FM, units of 2^-24: twice the 1.140 the first run measured, rounded up
FM_ARG_MAX = 0.9       # the bound holds for |arg z| <= 0.9 pi

# (K, Ta, Da, layout): "streams" is (steps, K) in memory, strides (K, 1) -- what the channeliser
# writes; "time" is (K, steps), strides (1, steps) -- taps written back to back
CASES = [(1, 1, 1, "time"), (1, 33, 4, "time"), (3, 8, 3, "streams"), (3, 8, 3, "time"), (64, 65, 8, "streams"),
         (1024, 17, 2, "streams"), (16, 256, 64, "streams"), (5, 1024, 1, "time")]
IDS = [f"K{K}-Ta{Ta}-Da{Da}-{lay}" for K, Ta, Da, lay in CASES]


def case_len(span):
    """Steps of a case's push: three full tiles of its form and a ragged tail."""
    return 3 * span + span // 3 + 1


def fm_seed(i):
    """The seed of case i's FM signal (test_demod_host.py checks each against the 0.9 pi condition)."""
    return 11 + i


def ceil_div(a, d):
    return -(-int(a) // int(d))


def steps(n0, n, Da):
    """Outputs of a push of n steps at count n0."""
    return max(0, ceil_div(n0 + n, Da) - ceil_div(n0, Da))


def step_indices(n0, n, Da):
    """The m of those outputs, Python ints."""
    return list(range(ceil_div(n0, Da), max(ceil_div(n0 + n, Da), ceil_div(n0, Da))))


def strides(layout, K, n):
    """(step_stride, stream_stride) of n steps of K streams in `layout`."""
    return (K, 1) if layout == "streams" else (1, n)


def lay(x, layout):
    """The (steps, K) array as the flat complex64 memory of `layout`."""
    x = np.asarray(x, dtype=np.complex64)
    return np.ascontiguousarray(x if layout == "streams" else x.T).reshape(-1)


def detect(x, n_first, modes, words):
    """d[i, s] for the (steps, K) stream whose step n_first + i is x[i], every earlier step 0."""
    x = np.asarray(x, dtype=np.complex128)
    K = x.shape[1]
    modes = np.broadcast_to(np.asarray(modes, dtype=np.int64), (K,))
    words = np.broadcast_to(np.asarray(words, dtype=np.int64), (K,))
    prev = np.vstack([np.zeros((1, K), np.complex128), x[:-1]])
    d = np.zeros(x.shape, dtype=np.float64)
    n = [(int(n_first) + i) % TWO32 for i in range(x.shape[0])]   # Python ints: exact
    for s in range(K):
        xs = x[:, s]
        if modes[s] == AM:
            d[:, s] = np.abs(xs)
        elif modes[s] == POWER:
            d[:, s] = xs.real ** 2 + xs.imag ** 2
        elif modes[s] == FM:
            z = xs * np.conj(prev[:, s])
            d[:, s] = np.where(z == 0, 0.0, np.angle(z) / np.pi)
        elif modes[s] == SSB:
            w = int(words[s]) % TWO32
            ph = np.array([(w * v) % TWO32 for v in n], dtype=np.float64)
            d[:, s] = (xs * np.exp(2j * np.pi * (ph / TWO32))).real
        else:
            raise ValueError(modes[s])
    return d


def ref_demod(x, n_first, modes, words, g, Da, ms):
    """a[m, s], m in ms (Python ints), from the (steps, K) stream starting at count n_first."""
    g = np.asarray(g, dtype=np.float64)
    d = detect(x, n_first, modes, words)
    at = np.array([int(m) * int(Da) - int(n_first) for m in ms], dtype=np.int64)   # d[m Da] in d's rows
    assert at.size == 0 or (at.min() >= 0 and at.max() < d.shape[0])
    out = np.zeros((at.size, d.shape[1]), dtype=np.float64)
    for s in range(d.shape[1]):
        out[:, s] = np.convolve(d[:, s], g)[at]                 # sum_k g[k] d[i - k], d = 0 before the start
    return out


def ref_push(x, n0, modes, words, g, Da):
    """All outputs of one push of x at count n0 (the past all zero)."""
    return ref_demod(x, n0, modes, words, g, Da, step_indices(n0, len(x), Da))


def d_max(mode, xmax):
    return {AM: xmax, SSB: xmax, POWER: xmax * xmax, FM: 1.0}[int(mode)]


def eps(mode, xmax):
    """The detector's error bound, the header's rule 6."""
    return {AM: 3 * U * xmax, POWER: 3 * U * xmax * xmax, SSB: 8 * U * xmax, FM: EPS_FM * U}[int(mode)]


def gate(g, mode, xmax):
    g = np.asarray(g, dtype=np.float64)
    s = np.abs(g).sum()
    return (g.size + 32) * U * s * d_max(mode, xmax) + s * eps(mode, xmax)


def gates(g, modes, xmax):
    """`gate` per stream, for a bank of mixed modes."""
    return np.array([gate(g, m, xmax) for m in modes])


def audio_taps(Ta, Da, seed=0):
    """Caller-supplied float32 audio taps with no small entries: |g[k]| in [0.5, 1], random signs
    (as tap_ref.solid_taps), so that every tap's term counts in the comparison."""
    rng = np.random.default_rng(1000 + Ta + 7 * Da + seed)
    return (rng.uniform(0.5, 1.0, Ta) * rng.choice([-1.0, 1.0], Ta)).astype(np.float32)


def noise_and_tones(n, K, seed):
    """(n, K) complex64: tap_ref.noise_and_tones per stream, |x| below about 1.3."""
    import tap_ref as tp
    return np.stack([tp.noise_and_tones(n, seed + 31 * s, tones=((0.013 + 0.0007 * s, 0.5), (-0.21, 0.25)))
                     for s in range(K)], axis=1)


def fm_signal(n, K, seed):
    """(n, K) complex64 of constant envelope: random audio (a smoothed uniform sequence of peak 1)
    at a peak deviation of 0.6 pi per step, plus noise of amplitude at most 0.05."""
    rng = np.random.default_rng(seed)
    audio = rng.uniform(-1.0, 1.0, (n + 7, K))
    audio = sum(audio[i:i + n] for i in range(8)) / 8.0
    audio /= np.abs(audio).max(axis=0)
    phase = np.cumsum(0.6 * np.pi * audio, axis=0)
    noise = 0.05 * rng.uniform(0.0, 1.0, (n, K)) * np.exp(2j * np.pi * rng.uniform(0.0, 1.0, (n, K)))
    return (np.exp(1j * phase) + noise).astype(np.complex64)


def fm_arg_ok(x):
    """Every |arg(x[n] conj(x[n-1]))| <= 0.9 pi on the float64 reference (the first step's product
    with the zero before the start is 0)."""
    x = np.asarray(x, dtype=np.complex128)
    z = x[1:] * np.conj(x[:-1])
    return bool(np.all(np.abs(np.angle(z)) <= FM_ARG_MAX * np.pi))


# ---------------------------------------------------------------- the rule in float32, bit for bit
# The header's rules 2 and 3 with every product, fused multiply-add, square root and sum rounded
# where the header says the kernel rounds (tests/f32_exact.py): a comparison with these is an
# equality, not a gate.  What the host cannot reproduce -- the device library's atan2f (FM) and
# sincospif at a general phase (SSB) -- is left out: FM gives its z and the predicate of its d = 0
# branch, SSB is modelled at the words whose phase is always a whole quarter turn.
QUARTER_WORDS = (0, 1 << 30, -(1 << 30), -(1 << 31))


def _parts(x):
    x = np.ascontiguousarray(x, dtype=np.complex64)
    return np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)


def power_f32(x):
    """POWER: d = fma(x.re, x.re, mul(x.im, x.im))."""
    import f32_exact as fx
    re, im = _parts(x)
    return fx.fma(re, re, fx.mul(im, im))


def am_f32(x):
    """AM: d = sqrt(fma(x.re, x.re, mul(x.im, x.im)))."""
    import f32_exact as fx
    return fx.sqrt(power_f32(x))


def ssb_quarter_f32(x, n_first, w):
    """SSB at a word of QUARTER_WORDS: r = exp(+2 pi i ((w n) mod 2^32) / 2^32) is exactly one of
    (1, 0), (0, 1), (-1, 0), (0, -1); d = fma(x.re, r.re, -mul(x.im, r.im)).  x is (n,) or (n, K)."""
    import f32_exact as fx
    assert int(w) in QUARTER_WORDS, w
    re, im = _parts(x)
    q = np.array([(((int(w) % TWO32) * ((int(n_first) + i) % TWO32)) % TWO32) >> 30 for i in range(re.shape[0])])
    q = q.reshape((-1,) + (1,) * (re.ndim - 1))
    r_re = np.broadcast_to(np.choose(q, [1.0, 0.0, -1.0, 0.0]).astype(np.float32), re.shape)
    r_im = np.broadcast_to(np.choose(q, [0.0, 1.0, 0.0, -1.0]).astype(np.float32), re.shape)
    return fx.fma(re, r_re, -fx.mul(im, r_im))


def fm_z_f32(x):
    """FM's z = x conj(p), p the step before (0 before the first): z.re = fma(x.re, p.re, mul(x.im,
    p.im)), z.im = fma(x.im, p.re, -mul(x.re, p.im)).  x is (n, K); returns (z.re, z.im)."""
    import f32_exact as fx
    re, im = _parts(x)
    p_re, p_im = np.vstack([np.zeros_like(re[:1]), re[:-1]]), np.vstack([np.zeros_like(im[:1]), im[:-1]])
    return fx.fma(re, p_re, fx.mul(im, p_im)), fx.fma(im, p_re, -fx.mul(re, p_im))


def fm_zero_f32(x):
    """Where z.re == z.im == 0 in float32 (x = 0, p = 0, or both products underflow): d is exactly 0."""
    z_re, z_im = fm_z_f32(x)
    return (z_re == 0) & (z_im == 0)


def modelled(mode, word=0):
    """Whether detect_f32 gives this mode (and word) wholly on the host."""
    return int(mode) in (AM, POWER) or (int(mode) == SSB and int(word) in QUARTER_WORDS)


def detect_f32(x, n_first, modes, words):
    """d[i, s] in float32 for the (steps, K) stream whose step n_first + i is x[i]; every stream
    must be `modelled`."""
    x = np.asarray(x, dtype=np.complex64)
    K = x.shape[1]
    modes = np.broadcast_to(np.asarray(modes, dtype=np.int64), (K,))
    words = np.broadcast_to(np.asarray(words, dtype=np.int64), (K,))
    d = np.zeros(x.shape, dtype=np.float32)
    for m in (AM, POWER):
        if (modes == m).any():
            d[:, modes == m] = (am_f32 if m == AM else power_f32)(x[:, modes == m])
    for s in np.nonzero(modes == SSB)[0]:
        d[:, s] = ssb_quarter_f32(x[:, s], n_first, words[s])
    assert all(modelled(m, w) for m, w in zip(modes, words))
    return d


def fir_f32(d, g, Da, n0, steps, first=None, block=1 << 15):
    """Rule 3 in float32: a[m, s] for the m with n0 <= m Da < n0 + steps, from the detected values d,
    float32 (n, K), d[i] being step first + i (default n0) and 0 before it.  Four partial sums a_j
    over the k = j (mod 4) in ascending k from +0, one fma(g[k], d, a_j) each, then add(add(a_0,
    a_1), add(a_2, a_3))."""
    import f32_exact as fx
    d = np.asarray(d)
    assert d.dtype == np.float32 and d.ndim == 2
    g = np.ascontiguousarray(g, dtype=np.float32)
    first = int(n0) if first is None else int(first)
    Ta = g.size
    dp = np.vstack([np.zeros((Ta - 1, d.shape[1]), np.float32), d])           # row i is step first - (Ta - 1) + i
    at = np.array([m * int(Da) - first + Ta - 1 for m in step_indices(n0, steps, Da)], dtype=np.int64)
    assert at.size == 0 or (at.min() >= Ta - 1 and at.max() < dp.shape[0])
    out = np.zeros((at.size, d.shape[1]), np.float32)
    rows = max(1, block // d.shape[1])
    for b in range(0, at.size, rows):                                        # (blocks that stay in the cache)
        i = at[b:b + rows]
        a = [np.zeros((i.size, d.shape[1]), np.float32) for _ in range(4)]
        for k in range(Ta):
            a[k & 3] = fx.fma(g[k], dp[i - k], a[k & 3])
        out[b:b + rows] = fx.add(fx.add(a[0], a[1]), fx.add(a[2], a[3]))
    return out


def model_push(x, n0, modes, words, g, Da):
    """All outputs of one push of x at count n0 (the past all zero), in float32: detect_f32, fir_f32."""
    return fir_f32(detect_f32(x, n0, modes, words), g, Da, n0, len(x))


def same(got, want):
    """The comparison of the exact tests: equal values, NaN equal to NaN, +0 equal to -0 (the header
    does not fix the sign of a zero sum), and no tolerance."""
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


def first_difference(got, want):
    """A line naming the first differing value and its bit patterns, for a failing comparison."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"shapes {got.shape} {want.shape}, types {got.dtype} {want.dtype}"
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    if not bad.any():
        return "equal"
    at = tuple(int(v) for v in np.argwhere(bad)[0])
    u = np.uint32 if got.dtype == np.float32 else np.uint64
    return (f"{int(bad.sum())} of {bad.size} differ, first at {at}: got {got[at]!r} ({int(got[at].view(u)):#x}), "
            f"want {want[at]!r} ({int(want[at].view(u)):#x})")
