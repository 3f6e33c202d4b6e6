"""The lane exchanges between inverse stages 2, 3 and 4 of the FC decimator (fc_kernels.hip:
xchg_54, xchg_32), as a numpy model of the exact instruction sequence, one wave of 64 lanes and
four registers per butterfly, written to the instructions' documented semantics:

  v_permlane32_swap a, b   lanes 32..63 of a exchange with lanes 0..31 of b
  v_permlane16_swap a, b   the odd 16-lane rows of a exchange with the even rows of b
                           (row 1 with row 0, row 3 with row 2)
  v_mov_b32_dpp d, s row_shr:n bank_mask:m   lane i of d takes lane i - n of s inside its 16-lane
                           row, where bit (i & 15) >> 2 of m is set; other lanes keep d
  ... row_shl:n            the same from lane i + n

The kernel swaps each dword of a complex value with the same sequence, so the model moves whole
elements.  Element numbers are those of test_fc_tables.test_fc_inverse_stages_2_to_4_are_wave_local:
slot i of the inverse array (before padding), butterfly t + 256 h of wave t >> 6."""
import numpy as np
import pytest

LANES = np.arange(64)


def permlane32_swap(a, b):
    a, b = a.copy(), b.copy()
    a[32:], b[:32] = b[:32].copy(), a[32:].copy()
    return a, b


def permlane16_swap(a, b):
    a, b = a.copy(), b.copy()
    for r in (0, 2):
        lo, hi = slice(16 * r, 16 * r + 16), slice(16 * r + 16, 16 * r + 32)
        a[hi], b[lo] = b[lo].copy(), a[hi].copy()
    return a, b


def mov_dpp(old, src, shift, bank_mask):
    """shift > 0: row_shr (from the lane `shift` below); < 0: row_shl (from above).  bound_ctrl
    off: a lane whose source falls outside its row keeps old."""
    out = old.copy()
    for i in LANES:
        j = (i & 15) - shift
        if (bank_mask >> ((i & 15) >> 2)) & 1 and 0 <= j < 16:
            out[i] = src[(i & ~15) + j]
    return out


def swap_row(a, b, sh):
    hi = 0xc if sh == 8 else 0xa
    return mov_dpp(a, b, sh, hi), mov_dpp(b, a, -sh, 0xf ^ hi)


def xchg_54(v):
    v = list(v)
    v[0], v[2] = permlane32_swap(v[0], v[2])
    v[1], v[3] = permlane32_swap(v[1], v[3])
    v[0], v[1] = permlane16_swap(v[0], v[1])
    v[2], v[3] = permlane16_swap(v[2], v[3])
    return v


def xchg_32(v):
    v = list(v)
    v[0], v[2] = swap_row(v[0], v[2], 8)
    v[1], v[3] = swap_row(v[1], v[3], 8)
    v[0], v[1] = swap_row(v[0], v[1], 4)
    v[2], v[3] = swap_row(v[2], v[3], 4)
    return v


def layout(stage, w, h):
    """Element held by (register a, lane l) of wave w's butterflies h at the start of a stage."""
    l = LANES
    base = 256 * w + 1024 * h
    if stage == 2:
        return [base + l + 64 * a for a in range(4)]
    if stage == 3:
        return [base + (l & 15) + 16 * a + 64 * (l >> 4) for a in range(4)]
    return [base + (l & 3) + 4 * a + 16 * ((l >> 2) & 3) + 64 * (l >> 4) for a in range(4)]


def test_primitives_follow_the_documented_semantics():
    a, b = LANES.copy(), 100 + LANES
    x, y = permlane32_swap(a, b)
    assert (x[:32] == a[:32]).all() and (x[32:] == b[:32]).all()
    assert (y[:32] == a[32:]).all() and (y[32:] == b[32:]).all()
    x, y = permlane16_swap(a, b)
    for r in range(4):
        s = slice(16 * r, 16 * r + 16)
        if r & 1:
            assert (x[s] == b[16 * (r - 1):16 * r]).all() and (y[s] == b[s]).all()
        else:
            assert (x[s] == a[s]).all() and (y[s] == a[16 * (r + 1):16 * (r + 2)]).all()
    d = mov_dpp(a, b, 4, 0xa)        # banks 1 and 3 of each row, from 4 lanes below
    for i in LANES:
        assert d[i] == (b[i - 4] if (i >> 2) & 1 else a[i])
    d = mov_dpp(a, b, -8, 0x3)       # banks 0 and 1, from 8 lanes above
    for i in LANES:
        assert d[i] == (b[i + 8] if (i & 15) < 8 else a[i])
    d = mov_dpp(a, b, 8, 0xf)        # every bank enabled: sources below the row keep old
    for i in LANES:
        assert d[i] == (b[i - 8] if (i & 15) >= 8 else a[i])


@pytest.mark.parametrize("Z", [8, 4])
def test_exchanges_carry_each_stage_layout_to_the_next(Z):
    NB = 8192 // Z // 1024
    for w in range(4):
        for h in range(NB):
            v = layout(2, w, h)
            v = xchg_54(v)
            for a in range(4):
                np.testing.assert_array_equal(v[a], layout(3, w, h)[a], f"stage 3 w={w} h={h} a={a}")
            v = xchg_32(v)
            for a in range(4):
                np.testing.assert_array_equal(v[a], layout(4, w, h)[a], f"stage 4 w={w} h={h} a={a}")


@pytest.mark.parametrize("Z", [8, 4])
def test_each_stage_holds_the_pinned_wave_local_element_set(Z):
    """The sets test_fc_inverse_stages_2_to_4_are_wave_local pins: per wave the same 256 NB
    elements at every stage, all with b0 = i >> 8 equal to (t >> 6) + 4 h; the butterflies
    h = 0, 1 of zoom 4 exchange independently."""
    NB = 8192 // Z // 1024
    bases = ((lambda u: (u & 63) + 256 * (u >> 6), 64),
             (lambda u: (u & 15) + 64 * ((u >> 4) & 3) + 256 * (u >> 6), 16),
             (lambda u: (u & 3) + 16 * ((u >> 2) & 3) + 64 * ((u >> 4) & 3) + 256 * (u >> 6), 4))
    for w in range(4):
        pinned = [{base(t) + 1024 * h + S * a for t in range(64 * w, 64 * w + 64)
                   for h in range(NB) for a in range(4)} for base, S in bases]
        held = []
        for h in range(NB):
            v2 = layout(2, w, h)
            v3 = xchg_54(v2)
            v4 = xchg_32(v3)
            held.append([v2, v3, v4])
            for v in (v2, v3, v4):
                assert all(((r >> 8) == w + 4 * h).all() for r in v)
        for s in range(3):
            got = set(np.concatenate([np.concatenate(held[h][s]) for h in range(NB)]).tolist())
            assert got == pinned[s] and len(got) == 256 * NB
        # the register a butterfly reads at each stage is the one the pinned address map gives
        for s, (base, S) in enumerate(bases):
            for h in range(NB):
                for a in range(4):
                    want = np.array([base(64 * w + l) + 1024 * h + S * a for l in LANES])
                    np.testing.assert_array_equal(held[h][s][a], want)
