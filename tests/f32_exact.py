"""float32 operations rounded once, in numpy: `mul`, `add`, `fma`, `sqrt` on float32 arrays, each the
correctly rounded (to nearest, ties to even) float32 result of the exact operation -- denormal
results, overflow to inf, inf / NaN propagation and the IEEE sign rules included.  What the
float32 models of the header's rules (demod_ref.fir_f32, tap_ref.tap_f32) are built from;
tests/test_f32_exact.py checks each against exact rational arithmetic.

mul, add: numpy's float32 operators round once.
sqrt:     the float64 square root of a float32, rounded to float32, is correctly rounded: 53 >=
          2 * 24 + 2, so the double rounding is harmless.
fma:      float32(float64(a) * float64(b) + float64(c)) rounds twice and is wrong (`fma_naive`,
          kept as the negative control).  `fma` rounds the float64 sum to odd first: the product is
          exact in float64 (48 bits), a TwoSum of product and addend gives the float64 sum s and its
          exact error e, and where e != 0 and s's last mantissa bit is even s moves one unit in its
          last place towards e.  A sum rounded to odd at 53 bits rounds to float32 (24 bits, fewer
          for a denormal result) as the exact sum does.  Nothing overflows or goes denormal in
          float64 on the way: |a b| is in [2^-298, 2^256) or 0."""
import numpy as np

F32, F64 = np.float32, np.float64


def _f32(a):
    a = np.asarray(a)
    assert a.dtype == F32, a.dtype
    return a


def mul(a, b):
    with np.errstate(all="ignore"):
        return np.multiply(_f32(a), _f32(b), dtype=F32)


def add(a, b):
    with np.errstate(all="ignore"):
        return np.add(_f32(a), _f32(b), dtype=F32)


def sqrt(a):
    with np.errstate(all="ignore"):
        return np.sqrt(_f32(a).astype(F64)).astype(F32)


def fma_naive(a, b, c):
    """Two roundings: NOT the fused multiply-add (the negative control of test_f32_exact.py)."""
    with np.errstate(all="ignore"):
        return (_f32(a).astype(F64) * _f32(b).astype(F64) + _f32(c).astype(F64)).astype(F32)


def fma(a, b, c):
    """float32(a b + c) with one rounding."""
    with np.errstate(all="ignore"):
        p = _f32(a).astype(F64) * _f32(b).astype(F64)          # exact
        c = np.broadcast_to(_f32(c).astype(F64), p.shape)
        s = p + c
        t = s - p
        e = (p - (s - t)) + (c - t)                            # TwoSum: p + c = s + e exactly (s finite)
        bits = np.array(s, dtype=F64, ndmin=1).view(np.int64)  # (a copy: s itself stays)
        fix = np.isfinite(s) & (e != 0) & ((bits & 1) == 0)    # (s = 0 has e = 0)
        # one unit in the last place towards e: away from zero where e has s's sign
        step = np.where((e > 0) == (s > 0), 1, -1)
        bits += np.where(fix, step, 0).reshape(bits.shape)
        return bits.view(F64).reshape(np.shape(s)).astype(F32)
