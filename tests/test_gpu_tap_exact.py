"""GPU checks of the channel taps (zfft_plan_taps; csrc/tap_kernels.hip) against the header's
arithmetic itself: tap_ref.tap_f32 (on tests/f32_exact.py) rounds where rule 7 of include/zfft.h
says the kernel rounds, on the table zfft_tap_table builds, so every comparison here is
`np.array_equal(got, want, equal_nan=True)` on complex64 -- +0 equal to -0, no tolerance.

The rotation is a device library call (sincospif) the host cannot reproduce at a general phase, so
the words are fw = 0 and words with (fw D) mod 2^30 == 0, where rot(m) is exactly a quarter turn
and the product a swap and a sign; such words still give a fully complex table (D = 32: fw = 2^25
odd).  This assumes sincospif exact at multiples of one half, which these tests are the first to
check on the device (profiles/tap/README.md)."""
import numpy as np
import pytest

import demod_ref as dr
import tap_ref as tp
from test_gpu_tap import _design, _form_span, _plan

pytestmark = pytest.mark.gpu
COMPARED = [0]


@pytest.fixture(scope="module", autouse=True)
def _gpu(zfft_lib):
    from pypanadapter_amd import device_count
    assert device_count() >= 1, "GPU tests need a HIP device"
    yield
    print(f"\nexact comparisons of the taps: {COMPARED[0]} values, none differing")


def equal(got, want, what):
    assert dr.same(got.real, want.real) and dr.same(got.imag, want.imag) and got.dtype == np.complex64, \
        f"{what}: re {dr.first_difference(got.real, want.real)}; im {dr.first_difference(got.imag, want.imag)}"
    COMPARED[0] += int(want.size)


def words_of(D):
    """fw = 0 and the quarter-turn word with a fully complex table, or 2^30 and -2^31 where D leaves
    only those."""
    q = tp.quarter_word(D)
    return [0, q] if q is not None else [0, 2 ** 30, -2 ** 31]


def open_all(plan, D, taps):
    """One slot per (fw, h); the tables the model runs on."""
    from pypanadapter_amd.engine import tap_table
    tabs = []
    for slot, (fw, h) in enumerate(taps):
        assert (fw * D) % 2 ** 30 == 0
        plan.tap_open(slot, fw / 2.0 ** 32, D, taps=h)              # (fs = 1)
        assert plan.tap_info(slot)["freq_word"] == fw
        tabs.append(tap_table(fw, h))
    return tabs


@pytest.mark.parametrize("D,T", tp.DT_TAPS)
def test_outputs_are_the_float32_rule(D, T):
    """test_gpu_tap's noise_and_tones push (two spans and a ragged tail), solid taps and the default
    design, at fw = 0 and at a quarter-turn word."""
    n = 2 * 512 + 301 + (T if T > 1024 else 0)
    x = tp.noise_and_tones(n, 7 + D)
    taps = [(fw, h) for fw in words_of(D) for h in (tp.solid_taps(T, 100 + D), _design(D, T))]
    with _plan(max_taps=8) as plan:
        assert _form_span(plan, 0, n, [(fw, D, T, 0) for fw, _ in taps]) == 512
        tabs = open_all(plan, D, taps)
        ys = plan.tap_push(x)
    assert len(ys) == len(taps)
    for (fw, h), c, y in zip(taps, tabs, ys):
        if fw % 2 ** 30 and T >= 3:
            assert np.abs(c.real[1:3]).min() > 0 and np.abs(c.imag[1:3]).min() > 0    # a fully complex table
        equal(y, tp.model_push(x, 0, fw, D, c), f"D={D} T={T} fw={fw}")


def test_cuts_and_a_late_count_are_the_float32_rule():
    D, T = 8, 65
    fw = tp.quarter_word(D)
    taps = [(0, tp.solid_taps(T, 3)), (fw, tp.solid_taps(T, 4))]
    cut = [1, D - 1, T - 1, 513, 1]
    n = sum(cut) + 700
    cut.append(n - sum(cut))
    x = tp.noise_and_tones(n, 23)
    n0 = 2 ** 32 - 100                                   # the phase wraps inside the push
    got = {}
    with _plan() as plan:
        tabs = open_all(plan, D, taps)
        for start in (0, n0):
            plan.tap_reset(start)
            got[start, "whole"] = plan.tap_push(x)
            plan.tap_reset(start)
            parts, at = [], 0
            for c in cut:
                parts.append(plan.tap_push(x[at:at + c]))
                at += c
            got[start, "cut"] = [np.concatenate(p) for p in zip(*parts)]
            assert plan.tap_state() == start + n
    for start in (0, n0):
        for s, ((w, h), c) in enumerate(zip(taps, tabs)):
            want = tp.model_push(x, start, w, D, c)
            equal(got[start, "whole"][s], want, f"whole at {start}, fw={w}")
            equal(got[start, "cut"][s], want, f"cut at {start}, fw={w}")


def test_cu8_is_the_float32_rule():
    """The loader's float32 values are exact ((b - 127.5) (1 / 127.5) in float32), so the model
    applies unchanged."""
    D, T, n = 8, 65, 2 * 512 + 301
    z = tp.noise_and_tones(n, 61)
    raw = np.clip(np.round(np.stack([z.real, z.imag], axis=1) / 1.5 * 127.5 + 127.5), 0, 255).astype(np.uint8).reshape(-1)
    x = tp.loader(raw, "cu8")
    assert np.array_equal(x.astype(np.complex64).astype(np.complex128), x)
    taps = [(0, _design(D, T)), (tp.quarter_word(D), tp.solid_taps(T, 6))]
    with _plan(in_dtype="cu8") as plan:
        tabs = open_all(plan, D, taps)
        a = plan.tap_push(raw[:2 * 333])
        b = plan.tap_push(raw[2 * 333:])
    for s, ((fw, h), c) in enumerate(zip(taps, tabs)):
        equal(np.concatenate([a[s], b[s]]), tp.model_push(x.astype(np.complex64), 0, fw, D, c), f"cu8 fw={fw}")
