"""The wave sum of the Welch kernels (zfft_kernels.hip: wave_sum) as a numpy float32 model of its
exact instruction sequence, one wave of 64 lanes, written to the instructions' documented
semantics (those of tests/test_fc_lane_exchange.py):

  v_permlane32_swap a, b   lanes 32..63 of a exchange with lanes 0..31 of b
  v_permlane16_swap a, b   the odd 16-lane rows of a exchange with the even rows of b
  v_add_f32_dpp d, s, s row_ror:8            lane i adds lane (i + 8) mod 16 of its row
  v_add_f32_dpp d, s, s row_shl:4 bound_ctrl lane i adds lane i + 4 of its row, 0 past its end
  v_add_f32_dpp d, s, s quad_perm:[2,3,0,1]  lane i adds lane i ^ 2
  v_add_f32_dpp d, s, s quad_perm:[1,0,3,2]  lane i adds lane i ^ 1

The kernel reads lane 0 alone.  Its value must have the bits of the xor butterfly 32, 16, 8, 4,
2, 1 (v += shfl_xor(v, m)), the form of before, so that rows do not change: the pairing is the
same at every step and float addition commutes."""
import numpy as np
import pytest

from test_fc_lane_exchange import permlane16_swap, permlane32_swap

LANES = np.arange(64)
F32 = np.float32


def add_dpp(v, src_lane):
    """v + v[src_lane(i)] per lane, float32; a lane whose source is outside its 16-lane row adds 0
    (bound_ctrl)."""
    out = v.copy()
    for i in LANES:
        j = src_lane(i & 15)
        out[i] = F32(v[i] + (v[(i & ~15) + j] if 0 <= j < 16 else F32(0)))
    return out


def wave_sum_model(v):
    v = np.asarray(v, F32)
    a, b = permlane32_swap(v, v)
    v = (a + b).astype(F32)
    a, b = permlane16_swap(v, v)
    v = (a + b).astype(F32)
    v = add_dpp(v, lambda r: (r + 8) & 15)       # row_ror:8
    v = add_dpp(v, lambda r: r + 4)              # row_shl:4, bound_ctrl
    v = add_dpp(v, lambda r: (r & ~3) + ((r & 3) ^ 2))  # quad_perm:[2,3,0,1]
    v = add_dpp(v, lambda r: (r & ~3) + ((r & 3) ^ 1))  # quad_perm:[1,0,3,2]
    return v


def xor_butterfly(v):
    v = np.asarray(v, F32).copy()
    for m in (32, 16, 8, 4, 2, 1):
        v = (v + v[LANES ^ m]).astype(F32)
    return v


def _inputs():
    rng = np.random.default_rng(20240521)
    for _ in range(200):
        yield rng.standard_normal(64).astype(F32)
    for _ in range(200):  # wide dynamic range
        yield (rng.standard_normal(64) * 10.0 ** rng.uniform(-8, 8, 64)).astype(F32)
    for _ in range(200):  # large cancellation: pairs of opposite sign at every butterfly distance
        big = (rng.standard_normal(64) * 1e6).astype(F32)
        m = int(rng.choice([32, 16, 8, 4, 2, 1]))
        v = big.copy()
        hi = (LANES & m) != 0
        v[hi] = -big[LANES ^ m][hi]
        yield (v + rng.standard_normal(64).astype(F32) * F32(1e-2)).astype(F32)
    for _ in range(50):   # the sum of a detrended-like block: mean far above the spread
        yield (F32(1e4) + rng.standard_normal(64).astype(F32)).astype(F32)


def test_butterfly_gives_every_lane_the_same_bits():
    """(what makes a lane-0 reduction enough: nothing reads another lane's different value)"""
    for v in _inputs():
        b = xor_butterfly(v)
        assert (b.view(np.uint32) == b.view(np.uint32)[0]).all()


def test_lane_0_has_the_butterflys_bits():
    n = 0
    for v in _inputs():
        got, want = wave_sum_model(v), xor_butterfly(v)
        assert got.view(np.uint32)[0] == want.view(np.uint32)[0], (n, got[0], want[0])
        n += 1
    assert n == 650


def test_first_two_steps_are_full_exchanges():
    """The permlane swaps of a value with its own copy give every lane its partner at distance
    32, then 16: after them all 64 lanes still agree with the butterfly, and after the row
    rotate too; from row_shl:4 on only the lanes 0..3 of each row do."""
    rng = np.random.default_rng(7)
    v = rng.standard_normal(64).astype(F32)
    a, b = permlane32_swap(v, v)
    s1 = (a + b).astype(F32)
    np.testing.assert_array_equal(s1, (v + v[LANES ^ 32]).astype(F32))
    a, b = permlane16_swap(s1, s1)
    s2 = (a + b).astype(F32)
    np.testing.assert_array_equal(s2, (s1 + s1[LANES ^ 16]).astype(F32))
    s3 = add_dpp(s2, lambda r: (r + 8) & 15)
    np.testing.assert_array_equal(s3, (s2 + s2[LANES ^ 8]).astype(F32))
    got, want = wave_sum_model(v), xor_butterfly(v)
    low = (LANES & 15) < 4
    np.testing.assert_array_equal(got[low].view(np.uint32), want[low].view(np.uint32))


@pytest.mark.parametrize("lane", [0, 5, 17, 63])
def test_a_single_nonzero_lane_reaches_lane_0(lane):
    v = np.zeros(64, F32)
    v[lane] = F32(3.25)
    assert wave_sum_model(v)[0] == F32(3.25)
