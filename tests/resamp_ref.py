"""Reference of the resampler bank: the rule of include/zfft.h (zfft_plan_resamp) in numpy float64,
written straight from the formulas with Python integers for every position -- never a call into
the library.

    y[m, s] = sum_{k<T} h[k L + p_m] x_s[i_m - k],   i_m = floor(m M / L),  p_m = m M mod L,

x the lanes' float32 values, 0 before the start of the count; a push of `steps` at count n0 emits
the m with n0 <= i_m < n0 + steps.  The error gate is the header's rule 7 (`gate`).

Below that, the same rule in float32 (model on tests/f32_exact.py): four partial sums over the
k = j (mod 4) in ascending k from +0, one fma each, joined (a_0 + a_1) + (a_2 + a_3), and the S16
format's one rounded product, rint and clamp -- for the comparisons that are equalities
(tests/test_gpu_resamp.py)."""
import numpy as np

U = 2.0 ** -24
F32, S16 = 0, 1
TIME, STREAMS = 0, 1

# (K, L, M, T, form) of the GPU cases
CASES = [(1, 1, 1, 1, TIME), (1, 3, 4, 8, TIME), (2, 160, 147, 16, TIME), (3, 2, 1, 5, TIME), (5, 1, 7, 24, TIME),
         (2, 5, 3, 1, TIME), (8, 16, 25, 32, STREAMS), (64, 147, 250, 32, STREAMS), (2048, 1, 2, 16, STREAMS),
         (70, 64, 25, 16, STREAMS)]
IDS = [f"K{K}-L{L}-M{M}-T{T}" for K, L, M, T, _ in CASES]
# the ratios whose default design's properties DESIGN.md states
DESIGN_RATIOS = [(16, 25), (147, 250), (3, 4), (160, 147), (2, 1), (1, 4), (1, 8), (3, 2)]


def case_len(span):
    """Steps of a case's push: two full spans of its form and a ragged part."""
    return 2 * span + span // 3 + 1


def ceil_div(a, d):
    return -(-int(a) // int(d))


def steps(n0, n, L, M):
    """Outputs of a push of n steps at count n0 (Python integers: n0 L passes 2^64)."""
    return max(0, ceil_div((int(n0) + int(n)) * L, M) - ceil_div(int(n0) * L, M))


def out_indices(n0, n, L, M):
    """The m of those outputs, Python ints."""
    return list(range(ceil_div(int(n0) * L, M), ceil_div((int(n0) + int(n)) * L, M)))


def positions(ms, L, M):
    """(i_m, p_m) of the outputs ms: Python ints and an int64 array."""
    return [int(m) * M // L for m in ms], np.array([int(m) * M % L for m in ms], dtype=np.int64)


def default_taps_per_phase(L, M):
    return 16 * ceil_div(max(L, M), L)


def group_delay(L, T):
    return (T * L - 1) / (2.0 * L)


def _rows(x, n_first, ms, L, M, T):
    """x with T - 1 zero steps before it, and for every m the row of x[i_m] in it with the phases."""
    i, ph = positions(ms, L, M)
    at = np.array([v - int(n_first) + T - 1 for v in i], dtype=np.int64)
    assert at.size == 0 or (at.min() >= T - 1 and at.max() < x.shape[0] + T - 1)
    return np.vstack([np.zeros((T - 1, x.shape[1]), x.dtype), x]), at, ph


def ref_resamp(x, n_first, h, L, M, ms):
    """y[m, s] in float64, m in ms (Python ints), from the (steps, K) lanes starting at count n_first."""
    x = np.asarray(x, dtype=np.float64)
    hp = np.asarray(h, dtype=np.float64).reshape(-1, L)       # hp[k, p] = h[k L + p]
    T = hp.shape[0]
    xp, at, ph = _rows(x, n_first, ms, L, M, T)
    out = np.zeros((at.size, x.shape[1]), dtype=np.float64)
    for k in range(T):
        out += hp[k, ph][:, None] * xp[at - k]
    return out


def ref_push(x, n0, h, L, M):
    """All outputs of one push of x at count n0 (the past all zero)."""
    return ref_resamp(x, n0, h, L, M, out_indices(n0, len(x), L, M))


def gate(h, L, xmax, ms=None, M=None):
    """Rule 7 per output: (T + 32) 2^-24 sum_k |h[k L + p]| max|x| (the worst phase without ms)."""
    s = np.abs(np.asarray(h, dtype=np.float64)).reshape(-1, L).sum(axis=0)
    T = np.asarray(h).size // L
    if ms is None:
        return (T + 32) * U * s.max() * xmax
    return ((T + 32) * U * xmax * s[positions(ms, L, M)[1]])[:, None]


def solid_taps(L, T, seed=0):
    """Caller-supplied float32 taps with no small entries: |h| in [0.5, 1] / T, random signs, so that
    every tap's term counts in a comparison."""
    rng = np.random.default_rng(2000 + 13 * L + T + seed)
    return (rng.uniform(0.5, 1.0, L * T) * rng.choice([-1.0, 1.0], L * T) / T).astype(np.float32)


def noise(n, K, seed):
    """(n, K) float32, uniform in [-1, 1]."""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, K)).astype(np.float32)


def response(h, nu):
    """|H(nu)| of the prototype at nu cycles per upsampled sample."""
    h = np.asarray(h, dtype=np.float64)
    return np.abs(np.exp(-2j * np.pi * np.outer(np.atleast_1d(nu), np.arange(h.size))) @ h)


def design_properties(h, L, M, dense=32):
    """(passband ripple in dB up to 0.24 / max(L, M), stopband attenuation in dB from 0.56 /
    max(L, M) to 0.5, worst |phase gain - 1|) of a prototype of gain L, on a frequency grid of
    `dense` points per 1 / len(h) (a side lobe is about that wide)."""
    q = max(L, M)
    hd = np.asarray(h, dtype=np.float64)
    n = dense * hd.size
    H = np.abs(np.fft.rfft(hd, n)) / L
    nu = np.arange(H.size) / n
    pb, sb = H[nu <= 0.24 / q], H[nu >= 0.56 / q]
    return (float(np.abs(20 * np.log10(pb)).max()), float(-20 * np.log10(sb.max())),
            float(np.abs(hd.reshape(-1, L).sum(axis=0) - 1.0).max()))


# ---------------------------------------------------------------- the rule in float32, bit for bit
def model_resamp(x, n_first, h, L, M, ms, block=1 << 15):
    """y[m, s] in float32, as rule 2 rounds: x float32 (n, K), step n_first + i being x[i]."""
    import f32_exact as fx
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2
    hp = np.ascontiguousarray(h, dtype=np.float32).reshape(-1, L)
    T = hp.shape[0]
    xp, at, ph = _rows(x, n_first, ms, L, M, T)
    out = np.zeros((at.size, x.shape[1]), np.float32)
    rows = max(1, block // x.shape[1])
    for b in range(0, at.size, rows):                           # (blocks that stay in the cache)
        i, p = at[b:b + rows], ph[b:b + rows]
        a = [np.zeros((i.size, x.shape[1]), np.float32) for _ in range(4)]
        for k in range(T):
            a[k & 3] = fx.fma(np.broadcast_to(hp[k, p][:, None], a[0].shape), xp[i - k], a[k & 3])
        out[b:b + rows] = fx.add(fx.add(a[0], a[1]), fx.add(a[2], a[3]))
    return out


def model_push(x, n0, h, L, M):
    """All outputs of one push of x at count n0 (the past all zero), in float32."""
    return model_resamp(x, n0, h, L, M, out_indices(n0, len(x), L, M))


def quantise(y, scale=32767.0):
    """Rule 4: int16 clamp(rint(float32(y scale))), NaN -> 0."""
    import f32_exact as fx
    y = np.asarray(y)
    assert y.dtype == np.float32
    v = fx.mul(y, np.float32(scale) * np.ones((), np.float32))
    with np.errstate(all="ignore"):
        q = np.clip(np.rint(v), -32768.0, 32767.0)
    return np.where(np.isnan(v), 0.0, q).astype(np.int16)


def same(got, want):
    """The comparison of the exact tests: equal values, NaN equal to NaN, +0 equal to -0 (the header
    does not fix the sign of a zero sum), and no tolerance."""
    got, want = np.asarray(got), np.asarray(want)
    nan = got.dtype.kind == "f"
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=nan)


def first_difference(got, want):
    """A line naming the first differing value and its bit patterns, for a failing comparison."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"shapes {got.shape} {want.shape}, types {got.dtype} {want.dtype}"
    bad = got != want
    if got.dtype.kind == "f":
        bad &= ~(np.isnan(got) & np.isnan(want))
    if not bad.any():
        return "equal"
    at = tuple(int(v) for v in np.argwhere(bad)[0])
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return (f"{int(bad.sum())} of {bad.size} differ, first at {at}: got {got[at]!r} ({int(got[at].view(u)):#x}), "
            f"want {want[at]!r} ({int(want[at].view(u)):#x})")
