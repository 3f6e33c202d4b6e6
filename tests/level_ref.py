"""Reference of the level bank: the rule of include/zfft.h (zfft_plan_level) in numpy float32,
written straight from the formulas with Python integers for every position -- never a call into
the library.  Every operation of the rule is a max, one correctly rounded division, one
subtraction, one fused multiply-add (tests/f32_exact.py) and one product, so the model is exact and
the comparisons of tests/test_gpu_level.py are equalities.

    P[b, s] = max over block b of m(key_s[n]),  m(v) = 0 for NaN, else min(|v|, 2^60)
    E[b, s] = max(P[b - H .. b, s])
    G[b, s] = min(gmax, target / max(E, floor)),  0 where squelch > 0 and E < squelch
    n = b B + i:  g = fma(i / B, min(G[b], G[b + 1]) - min(G[b - 1], G[b]), min(G[b - 1], G[b]))
    y[n, s] = g x_s[n]

on an absolute block grid, x and the key 0 before the start n_r; a bank at count N has emitted the
steps [n_r, emitted(N))."""
import numpy as np

F32 = np.float32
CAP = F32(2.0 ** 60)
TIME, STREAMS = 0, 1
DEFAULTS = dict(target=0.5, gmax=1e4, floor=1e-6, squelch=0.0)


def div(a, b):
    """float32 a / b rounded once (numpy's float32 division is IEEE's; test_level_host.py holds it
    to exact rationals)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == F32 and b.dtype == F32
    with np.errstate(all="ignore"):
        return np.divide(a, b, dtype=F32)


def emitted(N, n_r, B):
    """Rule 7, Python integers."""
    N, n_r, B = int(N), int(n_r), int(B)
    assert N >= n_r >= 0
    return max(n_r, B * (N // B - 1))


def steps(n0, n_r, n, B):
    """Steps a push of n at count n0 emits."""
    return emitted(int(n0) + int(n), n_r, B) - emitted(n0, n_r, B)


def mag(v):
    """Rule 3's m(v)."""
    v = np.asarray(v)
    assert v.dtype == F32
    with np.errstate(all="ignore"):
        return np.where(np.isnan(v), F32(0), np.minimum(np.abs(v), CAP)).astype(F32)


def gain(E, target, gmax, floor, squelch):
    """Rule 4 on float32 envelopes."""
    E = np.asarray(E)
    assert E.dtype == F32
    t, gm, fl, sq = F32(target), F32(gmax), F32(floor), F32(squelch)
    G = np.minimum(gm, div(np.broadcast_to(t, E.shape).astype(F32), np.maximum(E, fl)))
    if sq > 0:
        G = np.where(E < sq, F32(0), G)
    return G.astype(F32)


def blocks(key, n_r, B, H, target=0.5, gmax=1e4, floor=1e-6, squelch=0.0):
    """(b_first, P, E, G) of the blocks b_first = n_r // B .. the last one the (n, K) key, whose
    first row is step n_r, touches -- that one from what there is of it.  Rows are blocks."""
    key = np.asarray(key)
    assert key.dtype == F32 and key.ndim == 2
    n, K = key.shape
    b0 = int(n_r) // B
    lead = int(n_r) - b0 * B
    nb = max(1, -(-(lead + n) // B))
    m = np.zeros((nb * B, K), F32)
    m[lead:lead + n] = mag(key)
    P = m.reshape(nb, B, K).max(axis=1)
    Pz = np.vstack([np.zeros((H, K), F32), P])               # blocks before the start: peak 0
    E = Pz[H:].copy()
    for j in range(1, H + 1):
        E = np.maximum(E, Pz[H - j:H - j + nb])
    return b0, P, E, gain(E, target, gmax, floor, squelch)


def model_push(x, n_r, B, H, key=None, **par):
    """All the steps a bank started at n_r has emitted once the (n, K) float32 x (key: the same
    shape, or None for x itself) has been pushed, however it was cut: (emitted(n_r + n) - n_r, K)."""
    import f32_exact as fx
    x = np.asarray(x)
    assert x.dtype == F32 and x.ndim == 2
    n, K = x.shape
    outs = emitted(int(n_r) + n, n_r, B) - int(n_r)
    if outs <= 0:
        return np.zeros((0, K), F32)
    p = {**DEFAULTS, **par}
    b0, _, _, G = blocks(x if key is None else key, n_r, B, H, **p)
    G0 = gain(np.zeros((1, K), F32), **p)                    # block b0 - 1: E = 0
    Gz = np.vstack([G0, G])
    nb = G.shape[0]
    lo = np.minimum(Gz[:-1], Gz[1:])                          # g_lo of block b0 + j
    hi = np.minimum(G[:-1], G[1:])                            # g_hi of it, for the blocks that have a next one
    lead = int(n_r) - b0 * B
    at = lead + np.arange(outs)                               # on the axis from b0 B
    j, i = at // B, at % B
    assert j.max() < nb - 1                                   # emitted only where block b + 1 is complete
    with np.errstate(all="ignore"):
        d = np.subtract(hi[j], lo[j], dtype=F32)
    t = (i.astype(F32) / F32(B)).astype(F32)[:, None]
    g = fx.fma(np.broadcast_to(t, d.shape).astype(F32), d, lo[j])
    return fx.mul(g, x[:outs])


def meter(key, n_r, B, H, **par):
    """Rule 9 after the (n, K) key has been pushed: (E, G) of the newest complete block."""
    p = {**DEFAULTS, **par}
    key = np.asarray(key)
    K = key.shape[1]
    done = (int(n_r) + len(key)) // B - int(n_r) // B         # complete blocks from b0 on
    if done <= 0:
        E = np.zeros(K, F32)
        return E, gain(E, **p)
    _, _, E, G = blocks(key, n_r, B, H, **p)
    return E[done - 1], G[done - 1]


def noise(n, K, seed, lo_db=-100.0):
    """(n, K) float32: uniform noise whose amplitude steps by up to 100 dB every few dozen steps,
    each lane on its own schedule."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, (n, K))
    for s in range(K):
        at = 0
        while at < n:
            run = int(rng.integers(5, 120))
            x[at:at + run, s] *= 10.0 ** (rng.uniform(lo_db, 0.0) / 20.0)
            at += run
    return x.astype(F32)


def same(got, want):
    """Equal values, NaN equal to NaN, +0 equal to -0, and no tolerance."""
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


def first_difference(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"shapes {got.shape} {want.shape}, types {got.dtype} {want.dtype}"
    bad = (got != want) & ~(np.isnan(got) & np.isnan(want))
    if not bad.any():
        return "equal"
    at = tuple(int(v) for v in np.argwhere(bad)[0])
    return (f"{int(bad.sum())} of {bad.size} differ, first at {at}: got {got[at]!r} ({int(got[at].view(np.uint32)):#x}), "
            f"want {want[at]!r} ({int(want[at].view(np.uint32)):#x})")
