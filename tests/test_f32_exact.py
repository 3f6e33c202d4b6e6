"""CPU checks of tests/f32_exact.py: every operation against `fractions.Fraction` arithmetic rounded
to nearest-even into float32 (`round_f32`, integers only), on random operands over the whole
exponent range, the double-rounding family of the fused multiply-add, results in the denormal
range, results at the overflow threshold, and signed zeros, infinities and NaN.  The naive float64
multiply-add must FAIL the same check: that is asserted, as the negative control."""
import math
from fractions import Fraction

import numpy as np

import f32_exact as fx

F32 = np.float32


def round_f32(q):
    """The Fraction q != 0 rounded to nearest, ties to even, as a float32 (inf past the threshold)."""
    assert q != 0
    sign, q = (-1.0 if q < 0 else 1.0), abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    assert Fraction(2) ** e <= q < Fraction(2) ** (e + 1)
    e = max(e, -126)                                     # the denormals share the quantum 2^-149
    n = q / Fraction(2) ** (e - 23)
    lo = n.numerator // n.denominator
    rem = n - lo
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and lo & 1):
        lo += 1
    if lo * Fraction(2) ** (e - 23) >= Fraction(2) ** 128:
        return F32(sign * np.inf)
    return F32(sign * math.ldexp(lo, e - 23))           # lo <= 2^24: exact in a double and in a float32


def _fr(v):
    return Fraction(float(v))


def _same(got, want):
    """Bitwise the same float32 (one NaN is as good as another)."""
    got, want = F32(got), F32(want)
    if np.isnan(want):
        return bool(np.isnan(got))
    return got.tobytes() == want.tobytes()


def _mismatches(op, exact, args):
    """How many of the operand tuples (finite, exact result non-zero) op gets wrong."""
    got = op(*[np.array(a, dtype=F32) for a in zip(*args)])
    return sum(not _same(g, round_f32(exact(*map(_fr, t)))) for g, t in zip(got, args))


def _random(rng, n, lo=-149, hi=127):
    """float32 values over the whole exponent range, denormals included, random signs."""
    m = rng.integers(1 << 23, 1 << 24, n).astype(np.float64)
    v = np.ldexp(m, rng.integers(lo, hi + 1, n) - 23) * rng.choice([-1.0, 1.0], n)
    return v.astype(F32)                                  # (the low exponents round into denormals)


def _family(rng, n):
    """a = 1 + 2^-k, b = 1 + 2^-(24 - k): the product's 24-bit rounding is a tie that only the tiny
    addend decides."""
    k = rng.integers(1, 12, n)
    a = (1.0 + np.ldexp(1.0, -k)).astype(F32)
    b = (1.0 + np.ldexp(1.0, -(24 - k))).astype(F32)
    c = (np.ldexp(1.0, -rng.integers(60, 101, n)) * rng.choice([-1.0, 1.0], n)).astype(F32)
    return list(zip(a, b, c))


FMA = lambda a, b, c: a * b + c


def test_fma_on_the_double_rounding_family_and_the_naive_one_fails_it():
    rng = np.random.default_rng(1)
    args = _family(rng, 2000)
    assert _mismatches(fx.fma, FMA, args) == 0
    bad = _mismatches(fx.fma_naive, FMA, args)
    print(f"naive float64 multiply-add: {bad} of {len(args)} wrong on the family")
    assert bad > len(args) // 4                          # the negative control: the check has teeth


def test_fma_on_random_operands():
    rng = np.random.default_rng(2)
    n = 20000
    a, b = _random(rng, n), _random(rng, n)
    # an addend near the product's size (cancellation, ties), far below it, far above it
    scale = np.ldexp(1.0, rng.choice([0, 0, 0, -30, -60, 40], n))
    c = a.astype(np.float64) * b.astype(np.float64) * rng.uniform(-2.0, 2.0, n) * scale
    c = np.where(np.abs(c) < 2.0 ** 127, c, 1.0).astype(F32)
    args = [t for t in zip(a, b, c) if _fr(t[0]) * _fr(t[1]) + _fr(t[2]) != 0]
    assert len(args) > n - 100
    assert _mismatches(fx.fma, FMA, args) == 0
    wide = list(zip(_random(rng, n, -60, 60), _random(rng, n, -60, 60), _random(rng, n, -120, 120)))
    assert _mismatches(fx.fma, FMA, wide) == 0


def test_results_in_the_denormal_range_and_at_the_overflow_threshold():
    rng = np.random.default_rng(3)
    n = 4000
    # products and sums around 2^-149 .. 2^-120: denormal results, ties at the denormal quantum
    a, b = _random(rng, n, -80, -60), _random(rng, n, -80, -60)
    c = _random(rng, n, -149, -125)
    args = list(zip(a, b, c))
    got = fx.fma(a, b, c)
    assert (np.abs(got) < 2.0 ** -126).sum() > n // 4    # (the range is reached)
    assert _mismatches(fx.fma, FMA, args) == 0
    assert _mismatches(fx.mul, lambda p, q: p * q, list(zip(a, b))) == 0
    assert _mismatches(fx.add, lambda p, q: p + q, [t for t in zip(c, _random(rng, n, -149, -125)) if t[0] != -t[1]]) == 0
    # exact ties at the denormal quantum: (2 j + 1) 2^-150 rounds to the even neighbour
    j = np.arange(1, 200, dtype=np.float64)
    b = np.full(j.size, 2.0 ** -75, F32)                 # (2^-150 is no float32: the product makes it)
    a = ((2 * j + 1) * 2.0 ** -75).astype(F32)
    assert _mismatches(fx.fma, FMA, list(zip(a, b, rng.choice([2.0 ** -149, -2.0 ** -149, 2.0 ** -140], j.size).astype(F32)))) == 0
    assert _mismatches(fx.mul, lambda p, q: p * q, list(zip(a, b))) == 0
    # around the overflow threshold (2 - 2^-24) 2^127: below it the largest finite, from it on inf
    big = np.nextafter(F32(np.inf), F32(0))
    assert _same(fx.fma(F32(2.0 ** 64), F32(2.0 ** 63), big), np.inf)
    assert _same(fx.fma(big, F32(1), F32(2.0 ** 102)), big)             # under half a unit: stays
    assert _same(fx.fma(big, F32(1), F32(2.0 ** 103)), np.inf)          # the tie goes to the even side: inf
    assert _same(fx.fma(big, F32(1), np.nextafter(F32(2.0 ** 103), F32(0))), big)
    assert _same(fx.fma(F32(2.0 ** 64), F32(2.0 ** 64), F32(-2.0 ** 127)), F32(2.0 ** 127))   # the product alone is no overflow
    assert _same(fx.fma(F32(2.0 ** 64), F32(2.0 ** 64), -big), F32(2.0 ** 104))
    a, b = _random(rng, n, 60, 66), _random(rng, n, 60, 66)
    c = _random(rng, n, 120, 127)
    got = fx.fma(a, b, c)
    assert np.isinf(got).sum() > n // 8 and np.isfinite(got).sum() > n // 8
    assert _mismatches(fx.fma, FMA, list(zip(a, b, c))) == 0
    assert _mismatches(fx.mul, lambda p, q: p * q, list(zip(a, b))) == 0
    assert _mismatches(fx.add, lambda p, q: p + q, list(zip(c, _random(rng, n, 120, 127)))) == 0


def test_mul_add_sqrt_on_random_operands():
    rng = np.random.default_rng(4)
    n = 5000
    a, b = _random(rng, n), _random(rng, n)
    assert _mismatches(fx.mul, lambda p, q: p * q, list(zip(a, b))) == 0
    near = a.astype(np.float64) * rng.uniform(-2.0, 2.0, n)
    near = np.where(np.abs(near) < 2.0 ** 127, near, 1.0).astype(F32)
    assert _mismatches(fx.add, lambda p, q: p + q, [t for t in zip(a, near) if t[0] != -t[1]]) == 0
    # sqrt: r = round(sqrt(v)) iff v lies between the squares of the midpoints to r's neighbours
    v = np.abs(np.concatenate([a, _random(rng, 500, -149, -120), (rng.integers(1, 4096, 500) ** 2).astype(F32)]))
    r = fx.sqrt(v)
    assert r.dtype == F32
    for vi, ri in zip(v, r):
        q, ri = _fr(vi), F32(ri)
        dn, up = _fr(np.nextafter(ri, F32(0))), _fr(np.nextafter(ri, F32(np.inf)))
        lo, hi = ((_fr(ri) + dn) / 2) ** 2, ((_fr(ri) + up) / 2) ** 2
        assert lo <= q <= hi and (q != lo or not int(ri.view(np.uint32)) & 1) and (q != hi or not int(ri.view(np.uint32)) & 1), (vi, ri)
    assert np.array_equal(fx.sqrt(np.array([4.0, 2.0 ** -148, 2.0 ** 126], F32)), np.array([2.0, 2.0 ** -74, 2.0 ** 63], F32))


def test_signed_zeros_infinities_and_nan():
    z, nz, one, inf, nan = F32(0.0), F32(-0.0), F32(1.0), F32(np.inf), F32(np.nan)
    tiny = F32(2.0 ** -149)
    cases = [  # (a, b, c, fma)
        (z, one, z, z), (nz, one, nz, nz), (nz, one, z, z), (z, one, nz, z), (nz, nz, nz, z),
        (one, one, -one, z), (-one, one, one, z),            # an exact cancellation is +0
        (tiny, tiny, z, z), (-tiny, tiny, z, nz), (-tiny, tiny, nz, nz), (tiny, tiny, nz, z),   # underflow keeps the sign
        (tiny, F32(0.5), z, z), (tiny, F32(0.75), z, tiny), (tiny, F32(1.5), z, F32(2.0 ** -148)),   # ties to even
        (inf, one, one, inf), (inf, z, one, nan), (inf, one, -inf, nan), (one, one, -inf, -inf), (nan, one, one, nan),
        (one, one, nan, nan), (F32(2.0 ** 64), F32(2.0 ** 64), -inf, -inf), (F32(2.0 ** 64), F32(2.0 ** 64), z, inf),
    ]
    for a, b, c, want in cases:
        assert _same(fx.fma(a, b, c), want), (a, b, c, fx.fma(a, b, c), want)
    a, b, c, want = (np.array(col, dtype=F32) for col in zip(*cases))
    got = fx.fma(a, b, c)                                # and as one array
    assert got.dtype == F32 and all(_same(g, w) for g, w in zip(got, want))
    assert _same(fx.mul(nz, one), nz) and _same(fx.mul(-tiny, tiny), nz) and _same(fx.mul(inf, z), nan)
    assert _same(fx.mul(F32(2.0 ** 64), F32(2.0 ** 64)), inf) and _same(fx.mul(F32(2.0 ** -75), F32(2.0 ** -75)), z)
    assert _same(fx.add(nz, nz), nz) and _same(fx.add(nz, z), z) and _same(fx.add(one, -one), z) and _same(fx.add(inf, -inf), nan)
    assert _same(fx.sqrt(z), z) and _same(fx.sqrt(nz), nz) and _same(fx.sqrt(inf), inf) and _same(fx.sqrt(-one), nan)
    assert _same(fx.sqrt(tiny), F32(2.0 ** -74.5))
    assert fx.fma(np.ones((3, 2), F32), np.ones(2, F32), F32(1)).shape == (3, 2)     # broadcasting
