"""GPU checks of the row history (zfft_plan_history: pushed rows kept on the device as float32 or
as 16- / 8-bit codes and re-reduced to any window) against history_ref, the rule of
include/zfft.h in numpy (pinned on the CPU by test_history_host.py).  What the store returns must
equal the reference quantiser bit for bit; the MAX and MIN of a view must equal the float32
reference over the unpacked rows bit for bit (-0.0 and 0.0 compare equal, as the rule leaves
them).  MEAN is held to conftest.assert_row_close, the project's row gate, against the float64
rule over the unpacked rows: 1e-3 dB within 100 dB of a line's peak and 1e-5 of the peak
amplitude.  The margin is the viewport test's, and so is the arithmetic: the device adds at most
four float32 terms before every sum goes on in float64, so its error is that of 10^(v/20) in
float32 (an argument rounding of 1.3e-6 relative at -160 dB, 1.1e-5 dB, plus the function's ulp).
Worst figures seen on an MI355X (printed by every MEAN check, kept in profiles/history/README.md):
max |ddB| 1.08e-5, max |d amp| / peak 4.8e-7."""
import ctypes
import functools

import numpy as np
import pytest

import history_ref as hr
import viewport_ref as vr
from conftest import assert_row_close, row_errors

pytestmark = pytest.mark.gpu
FS = 2.4e6
LO, HI = -150.0, -50.0  # the store's levels: the rows span -160 .. -40, so both clamps are hit
WHOLE, SLICED = 1, 2
WORST = [0.0, 0.0]


def _kind(plan):
    hook = plan.lib.zfft__plan_history_form
    hook.argtypes, hook.restype = [ctypes.c_void_p], ctypes.c_int
    return hook(plan._plan)


def same(got, ref, what=""):
    """Equal as float32 values, NaN in the same places (-0.0 == 0.0)."""
    np.testing.assert_array_equal(np.asarray(got), np.asarray(ref, dtype=np.float32), err_msg=what)


def same_bits(got, ref, what=""):
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=what)
    ok = ~np.isnan(ref)
    np.testing.assert_array_equal(got[ok].view(np.uint32), ref[ok].view(np.uint32), err_msg=what)


def mean_close(got, ref, what=""):
    """Every line of got (float32) against the float64 rule through the row gate; NaN and the
    infinities must sit in the same cells (the gate itself looks at finite reference values)."""
    got, ref = np.atleast_2d(got), np.atleast_2d(ref)
    assert got.shape == ref.shape, what
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=what)
    np.testing.assert_array_equal(np.isinf(got), np.isinf(ref), err_msg=what)
    for i, (a, b) in enumerate(zip(got, ref)):
        ok = np.isfinite(b)
        if not ok.any():
            continue
        ddb, damp = row_errors(a[ok], b[ok])
        WORST[0], WORST[1] = max(WORST[0], ddb), max(WORST[1], damp)
        print(f"history mean {what} line {i}: max|ddB|={ddb:.3e} max|damp|={damp:.3e} "
              f"(worst so far {WORST[0]:.3e} {WORST[1]:.3e})")
        assert_row_close(a[ok], b[ok], f"{what} line {i}")


def compare(det, got, ref, what=""):
    (mean_close if det == "mean" else same)(got, ref, what)


# name: (n_fft, n_win, in_dtype, (col0, col1, width), rows_per_line, rows) -- the viewport test's
# geometries, the display's col0 moved to 3 so that no tile starts on a 16-byte boundary
GEOMETRIES = {
    "identity": (64, 64, "complex64", (0, 64, 64), 1, 5),
    "short_real_rows": (1024, 301, "f32", (5, 150, 7), 2, 5),
    "one_pixel": (512, 512, "complex64", (0, 512, 1), 3, 7),
    "display_8192_to_1920": (8192, 8192, "complex64", (3, 8192, 1920), 1, 3),
    "tile_seam": (1024, 1024, "complex64", (3, 1003, 300), 2, 6),
    "wide_buckets": (1024, 1024, "complex64", (0, 1024, 3), 1, 2),
    "four_waves_a_group": (128, 128, "complex64", (0, 128, 32), 20, 70),
    # (not among the viewport's: a bucket of 1998 columns folds onto the lane's accumulators in every format)
    "a_bucket_wider_than_a_wave": (4096, 4096, "complex64", (5, 4001, 2), 2, 4),
}
F32_ON = ("identity", "short_real_rows", "a_bucket_wider_than_a_wave")


@functools.lru_cache(maxsize=None)
def _rows(name, inf):
    """Seeded uniform rows over -160 .. -40 with the specials planted, levels beyond both ends of
    the store's range, and every column outside the window (the tail beyond the row length too)
    poisoned."""
    N, W, dtype, geo, m, count = GEOMETRIES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    rows = rng.uniform(-160.0, -40.0, (count, W)).astype(np.float32)
    rows[-1, geo[0]] = -155.0
    rows[-1, geo[1] - 1] = -45.0
    assert vr.plant_specials(rows, geo, m, inf=inf) >= 1
    n = 151 if dtype == "f32" else W
    vr.poison_outside(rows, n, geo)
    assert (rows[:, geo[0]:geo[1]] < LO).any() and (rows[:, geo[0]:geo[1]] > HI).any()
    rows.setflags(write=False)
    return rows, n


@functools.lru_cache(maxsize=None)
def _kept(name, inf, fmt):
    rows, n = _rows(name, inf)
    kept = hr.stored(rows, fmt, LO, HI)
    kept.setflags(write=False)
    return kept


# ---------------------------------------------------------------- 1. round trip
@pytest.mark.parametrize("fmt", ["f32", "u16", "u8"])
@pytest.mark.parametrize("name", ["identity", "short_real_rows"])
def test_round_trip(name, fmt):
    from pypanadapter_amd import ZoomFFT
    N, W, dtype, geo, m, count = GEOMETRIES[name]
    rows, n = _rows(name, True)
    with ZoomFFT(N, 1, FS, n_win=W, in_dtype=dtype) as plan:
        assert plan.row_length == n
        plan.set_timing(True)
        plan.set_history(8, fmt, LO, HI)
        assert plan.history_shape() == (8, n, fmt) and plan.history_state() == (0, 0)
        plan.history_push(rows)
        assert plan.launch_names() == ["history_pack"] and len(plan.timings()) == 1
        assert plan.history_state() == (count, 0)
        got = plan.history_rows(0, count)
        assert plan.launch_names() == ["history_unpack"]
        assert got.shape == (count, W) and np.isnan(got[:, n:]).all()
        same_bits(got[:, :n], _kept(name, True, fmt)[:, :n], f"{name} {fmt}")
        if fmt == "f32":
            same_bits(got[:, :n], rows[:, :n], "f32 returns the input")
        else:
            K = hr.KMAX[fmt]
            codes = hr.pack(rows[:, :n], fmt, LO, HI)
            assert codes.min() == 0 and codes[codes > 0].min() == 1 and codes.max() == K + 1  # NaN and both clamps
        if dtype == "f32":  # cropped rows (as rows() returns them) are padded on the host
            plan.history_reset()
            plan.history_push(rows[:, :n])
            same_bits(plan.history_rows(0, count)[:, :n], got[:, :n], "cropped")


# ---------------------------------------------------------------- 2. the ring
@pytest.mark.parametrize("fmt", ["f32", "u8"])
def test_ring(fmt):
    from pypanadapter_amd import ZoomFFT
    rows = np.random.default_rng(12).uniform(-160.0, -40.0, (32, 64)).astype(np.float32)
    kept = hr.stored(rows, fmt, LO, HI)
    with ZoomFFT(64, 1, FS, n_win=64) as plan:
        plan.set_history(7, fmt, LO, HI)
        for at in (0, 3, 6, 9):
            plan.history_push(rows[at:at + 3])
        assert plan.history_state() == (12, 5)
        same_bits(plan.history_rows(5, 7), kept[5:12], "rows 5..11")
        same_bits(plan.history_rows(9, 2), kept[9:11], "rows 9, 10")
        for first, count in ((4, 1), (4, 8), (5, 8), (11, 2), (12, 1), (-1, 2), (5, 0)):
            with pytest.raises(ValueError):
                plan.history_rows(first, count)
        plan.history_push(rows[12:32])  # one push of 20 rows keeps its last 7
        assert plan.history_state() == (32, 25)
        same_bits(plan.history_rows(25, 7), kept[25:32], "the last 7 of 20")
        with pytest.raises(ValueError):
            plan.history_rows(24, 1)
        plan.history_reset()
        assert plan.history_state() == (0, 0)
        with pytest.raises(ValueError):
            plan.history_rows(0, 1)
        plan.history_push(rows[:2])
        assert plan.history_state() == (2, 0)
        same_bits(plan.history_rows(0, 2), kept[:2], "after the reset")


# ---------------------------------------------------------------- 3. views
VIEW_CASES = [(name, fmt) for name in GEOMETRIES for fmt in (("f32",) if name in F32_ON else ()) + ("u16", "u8")]


@pytest.mark.parametrize("det", vr.DETECTORS)
@pytest.mark.parametrize("name,fmt", VIEW_CASES)
def test_view(name, fmt, det):
    """The window over every stored row.  Three rows pushed before them put the window's first
    slot at 3, so the rows wrap the ring's end (capacity = the rows of the window)."""
    from pypanadapter_amd import ZoomFFT
    N, W, dtype, geo, m, count = GEOMETRIES[name]
    inf = det != "mean"
    rows, n = _rows(name, inf)
    kept = _kept(name, inf, fmt)
    lines = count // m
    with ZoomFFT(N, 1, FS, n_win=W, in_dtype=dtype) as plan:
        plan.set_timing(True)
        plan.set_history(count, fmt, LO, HI)
        plan.history_push(rows[[0, 0, 0]])
        plan.history_push(rows)
        assert plan.history_state() == (count + 3, 3)
        got = plan.history_view(3, lines, geo[2], m, det, geo[0], geo[1])
        assert got.shape == (lines, geo[2]) and got.dtype == np.float32
        assert _kind(plan) == WHOLE and plan.launch_names() == ["history_view"] and len(plan.timings()) == 1
        ref = hr.ref_view(kept, 3, n, 3, lines, geo, det, m)
        assert np.isfinite(ref).any()
        compare(det, got, ref, f"{name} {fmt} {det}")


# ---------------------------------------------------------------- 4. a window partly outside the store
@pytest.mark.parametrize("fmt", ["f32", "u16", "u8"])
@pytest.mark.parametrize("det", vr.DETECTORS)
def test_window_partly_outside_the_store(fmt, det):
    from pypanadapter_amd import ZoomFFT
    geo = (1, 63, 20)
    rows = np.random.default_rng(44).uniform(-160.0, -40.0, (12, 64)).astype(np.float32)
    rows[8, 30] = np.nan
    kept = hr.stored(rows, fmt, LO, HI)[5:]
    with ZoomFFT(64, 1, FS, n_win=64) as plan:
        plan.set_history(7, fmt, LO, HI)
        for at in (0, 3, 6, 9):
            plan.history_push(rows[at:at + 3])
        assert plan.history_state() == (12, 5)
        got = plan.history_view(3, 6, 20, 2, det, geo[0], geo[1])
        ref = hr.ref_view(kept, 5, 64, 3, 6, geo, det, 2)
        # rows 3, 4 | 5, 6 | 7, 8 (slots 0, 1: the wrap lies before it) | 9, 10 | 11, 12 | 13, 14
        assert np.isnan(got[0]).all() and np.isnan(got[4]).all() and np.isnan(got[5]).all()
        assert np.isfinite(got[1:4]).sum() >= 59
        compare(det, got, ref, f"{fmt} {det}")
        # first = 6: the line of rows 6, 7 lies in slots 6, 0 and straddles the ring's wrap
        got = plan.history_view(6, 3, 20, 2, det, geo[0], geo[1])
        compare(det, got, hr.ref_view(kept, 5, 64, 6, 3, geo, det, 2), f"{fmt} {det} across the wrap")
        assert np.isfinite(got[0]).sum() >= 19
        # a negative first: NaN lines and no error
        got = plan.history_view(-3, 5, 20, 2, det, geo[0], geo[1])
        compare(det, got, hr.ref_view(kept, 5, 64, -3, 5, geo, det, 2), f"{fmt} {det} negative first")
        assert np.isnan(got[:4]).all() and np.isfinite(got[4]).all()
        assert np.isnan(plan.history_view(-1000, 4, 20, 2, det, geo[0], geo[1])).all()
        assert np.isnan(plan.history_view(12, 4, 20, 1, det, geo[0], geo[1])).all()


# ---------------------------------------------------------------- 5. groups cut into slices
@functools.lru_cache(maxsize=None)
def _slice_rows():
    rows = np.random.default_rng(3000).uniform(-160.0, -40.0, (6000, 128)).astype(np.float32)
    rows[17, 5] = rows[4000, 64] = np.nan
    rows.setflags(write=False)
    kept = hr.stored(rows, "u8", LO, HI)
    kept.setflags(write=False)
    return rows, kept


@pytest.mark.parametrize("det", ["max", "mean"])
def test_groups_cut_into_slices(det):
    from pypanadapter_amd import ZoomFFT
    rows, kept = _slice_rows()
    geo = (0, 128, 16)
    with ZoomFFT(128, 1, FS, n_win=128) as plan:
        plan.set_timing(True)
        plan.set_history(6000, "u8", LO, HI)
        plan.history_push(rows)
        got = plan.history_view(0, 2, 16, 3000, det)
        assert _kind(plan) == SLICED and plan.launch_names() == ["history_view", "history_finish"]
        assert len(plan.timings()) == 2
        compare(det, got, hr.ref_view(kept, 0, 128, 0, 2, geo, det, 3000), f"sliced {det}")
        assert np.isnan(got[0, 0]) == (det == "mean") and np.isnan(got[1, 8]) == (det == "mean")
        # a sliced line that is not in the store is NaN from the finishing launch
        got = plan.history_view(3000, 2, 16, 3000, det)
        assert _kind(plan) == SLICED and np.isnan(got[1]).all()
        compare(det, got, hr.ref_view(kept, 0, 128, 3000, 2, geo, det, 3000), f"sliced {det}, second line outside")
        got = plan.history_view(0, 2, 16, 1, det)
        assert _kind(plan) == WHOLE and plan.launch_names() == ["history_view"]
        compare(det, got, hr.ref_view(kept, 0, 128, 0, 2, geo, det, 1), f"whole {det}")


# ---------------------------------------------------------------- 6. render
def test_render_equals_the_viewport_render():
    from pypanadapter_amd import ZoomFFT
    rows = np.random.default_rng(66).uniform(-160.0, -40.0, (14, 128)).astype(np.float32)
    rows[4, 40] = np.nan
    with ZoomFFT(128, 1, FS, n_win=128) as plan:
        plan.waterfall_colormap("Tropical")
        plan.waterfall_levels(LO, HI)
        plan.set_history(16, "u8", LO, HI)
        plan.history_push(rows)
        # lines of rows 2..13 (m = 3) and a line past rows_seen: alpha 0
        rgba = plan.history_render(2, 5, 30, 3, "max", 4, 124)
        assert rgba.shape == (5, 30, 4) and rgba.dtype == np.uint8
        assert not rgba[4, :, 3].any() and (rgba[:4, :, 3] == 255).all()
        plan.set_viewport(4, 30, 4, 124, "max", 3)
        plan.viewport_push(plan.history_rows(2, 12))
        np.testing.assert_array_equal(rgba[:4], plan.viewport_render(np.empty((4, 30, 4), np.uint8)))
        img = plan.history_view(2, 4, 30, 3, "max", 4, 124)
        same(img, plan.viewport_image(), "view == viewport image")
        out = np.empty((4, 30, 4), np.uint8)
        assert plan.history_render(2, 4, 30, 3, "max", 4, 124, out=out) is out
        np.testing.assert_array_equal(out, rgba[:4])
        with pytest.raises(ValueError):
            plan.history_render(2, 4, 30, 3, "max", 4, 124, out=np.empty((4, 30, 3), np.uint8))


# ---------------------------------------------------------------- 7. replay into the live viewport
@pytest.mark.parametrize("det", vr.DETECTORS)
def test_replay_into_the_live_viewport(det):
    from pypanadapter_amd import ZoomFFT
    rows = np.random.default_rng(77).uniform(-160.0, -40.0, (30, 128)).astype(np.float32)
    rows[22, 50] = np.nan
    win = (8, 30, 4, 124, det, 5)

    def check_equal(a, b, what):
        assert a.viewport_state() == b.viewport_state(), what
        compare(det, a.viewport_image(), b.viewport_image().astype(np.float64), what + " image")
        for k, (ta, tb) in enumerate(zip(a.viewport_traces(), b.viewport_traces())):
            compare(det, ta, tb.astype(np.float64), f"{what} trace {k}")

    with ZoomFFT(128, 1, FS, n_win=128) as plan, ZoomFFT(128, 1, FS, n_win=128) as fresh:
        plan.set_viewport(4, 16)         # the geometry before the zoom
        plan.set_history(22, "u8", LO, HI)
        plan.viewport_push(rows[:25])
        plan.history_push(rows[:25])
        assert plan.history_state() == (25, 3)
        plan.set_viewport(*win)
        plan.history_replay_viewport(0)
        kept = plan.history_rows(3, 22)
        same_bits(kept, hr.stored(rows[3:25], "u8", LO, HI), "the replayed rows")
        fresh.set_viewport(*win)
        fresh.viewport_push(kept)
        assert plan.viewport_state() == (22, 4, 2)
        check_equal(plan, fresh, "after the replay")
        for r in rows[25:30]:  # live rows carry on in both
            plan.history_push(r)
            plan.viewport_push(r)
            fresh.viewport_push(r)
        assert plan.viewport_state() == (27, 5, 2) and plan.history_state() == (30, 8)
        check_equal(plan, fresh, "five live rows later")
        # from a later row on: only what follows it
        plan.history_replay_viewport(20)
        fresh.viewport_reset()
        fresh.viewport_push(plan.history_rows(20, 10))
        check_equal(plan, fresh, "replay from row 20")
        # needs both features
        plan.set_viewport(0, 0)
        with pytest.raises(ValueError):
            plan.history_replay_viewport(0)
        with pytest.raises(ValueError):
            fresh.history_replay_viewport(0)


# ---------------------------------------------------------------- 8. device rows on the same stream
def test_device_rows_pushed_on_the_same_stream():
    """process_device into a torch buffer, then history_push_device on the same stream without a
    host wait in between, then a view: equal to the host-pushed result."""
    import torch
    from pypanadapter_amd import ZoomFFT
    F, L, W = 4, 256, 64
    rng = np.random.default_rng(88)
    x = (rng.standard_normal((F, L)) + 1j * rng.standard_normal((F, L))).astype(np.complex64) * 1e-3
    dev = torch.device("cuda:0")
    xd = torch.from_numpy(x.view(np.float32).reshape(F, L, 2)).to(dev)
    with ZoomFFT(64, 1, FS, n_win=W) as plan:
        host = plan.rows(x)
        lo, hi = float(np.floor(host.min())) + 2.0, float(np.ceil(host.max())) - 2.0  # both clamps are hit
        plan.set_history(8, "u8", lo, hi)
        rows = torch.empty((F, W), device=dev, dtype=torch.float32)
        img = torch.empty((2, 16), device=dev, dtype=torch.float32)
        st = torch.cuda.current_stream().cuda_stream
        plan.process_device(xd.data_ptr(), L, F, rows.data_ptr(), st)
        plan.history_push_device(rows.data_ptr(), F, st)
        plan.history_view_device(img.data_ptr(), 0, 2, 16, 2, "max", stream=st)
        got = plan.history_view(0, 2, 16, 2, "max")
        back = torch.empty((F, W), device=dev, dtype=torch.float32)
        plan.history_read_device(0, F, back.data_ptr(), st)
        torch.cuda.synchronize()
        dev_rows = rows.cpu().numpy()
        kept = hr.stored(dev_rows, "u8", lo, hi)
        same_bits(back.cpu().numpy(), kept, "read_device")
        same(got, hr.ref_view(kept, 0, W, 0, 2, (0, 64, 16), "max", 2), "device-pushed rows")
        same(img.cpu().numpy(), got, "view_device")
        assert np.isfinite(got).all() and plan.history_state() == (4, 0)
        plan.history_reset()
        plan.history_push(dev_rows)
        assert plan.history_view(0, 2, 16, 2, "max").tobytes() == got.tobytes()


# ---------------------------------------------------------------- 9. validation, off, lifecycle
def test_validation_and_off():
    from pypanadapter_amd import ZoomFFT, _lib
    rows = np.random.default_rng(9).uniform(-160.0, -40.0, (4, 128)).astype(np.float32)
    with ZoomFFT(128, 1, FS, n_win=128) as plan:
        lib, h = plan.lib, plan._plan
        cap, cols, fmt = ctypes.c_int64(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
        assert lib.zfft_history_shape(h, ctypes.byref(cap), ctypes.byref(cols), ctypes.byref(fmt)) == _lib.ZFFT_EINVAL
        assert cap.value == 0
        off_calls = (plan.history_shape, plan.history_state, plan.history_reset, lambda: plan.history_push(rows),
                     lambda: plan.history_push_device(8, 1), lambda: plan.history_rows(0, 1),
                     lambda: plan.history_read_device(0, 1, 8), lambda: plan.history_view(0, 1, 16),
                     lambda: plan.history_view_device(8, 0, 1, 16), lambda: plan.history_render(0, 1, 16),
                     plan.history_replay_viewport)
        for call in off_calls:
            with pytest.raises(ValueError):
                call()
        # a plan with the store off reports the timing names it always did
        plan.set_timing(True)
        plan.set_viewport(4, 16)
        plan.viewport_push(rows[0])
        assert plan.launch_names() == ["view_lines"]
        plan.set_viewport(0, 0)
        nan, inf = float("nan"), float("inf")
        for bad in ((-1, 2, LO, HI), (4, 3, LO, HI), (4, -1, LO, HI), (4, 2, HI, LO), (4, 1, LO, LO), (4, 2, nan, HI),
                    (4, 1, LO, nan), (4, 2, -inf, HI), (4, 2, LO, inf)):
            assert lib.zfft_plan_history(h, *bad) == _lib.ZFFT_EINVAL, bad
        with pytest.raises(ValueError):
            plan.set_history(4, "u4")
        with pytest.raises(ValueError):
            plan.history_state()  # a refused enable leaves the store off
        assert lib.zfft_plan_history(h, 4, 0, nan, nan) == _lib.ZFFT_OK  # F32 ignores the levels
        assert plan.history_shape() == (4, 128, "f32")
        plan.set_history(4, "u8", LO, HI)
        plan.history_push(rows[:3])
        # (first, lines, width, rows_per_line, detector, col0, col1)
        W = _lib.zfft_history_window
        img = np.empty(8192 * 4, np.float32)
        for first, lines, width, m, det, c0, c1 in ((0, 1, 65, 1, 0, 0, 64), (0, 0, 16, 1, 0, 0, 128),
                                                    (0, 8193, 1, 1, 0, 0, 128), (0, 1, 16, 0, 0, 0, 128),
                                                    (0, 1, 16, 65537, 0, 0, 128), (0, 1, 16, 1, 0, 0, 129),
                                                    (0, 1, 16, 1, 3, 0, 128), (0, 1, 16, 1, -1, 0, 128),
                                                    (0, 1, 16, 1, 0, -1, 128), (0, 1, 16, 1, 0, 64, 64),
                                                    (0, 1, 0, 1, 0, 0, 128)):
            w = W(first, m, lines, c0, c1, width, det)
            assert lib.zfft_history_view(h, ctypes.byref(w), img.ctypes.data) == _lib.ZFFT_EINVAL, (first, lines, width)
        with pytest.raises(ValueError):
            plan.history_view(0, 1, 16, detector="median")
        w = W(0, 65536, 8192, 0, 128, 4, 2)  # the limits themselves: every line outside the store
        assert lib.zfft_history_view(h, ctypes.byref(w), img.ctypes.data) == _lib.ZFFT_OK and np.isnan(img).all()
        with pytest.raises(ValueError):
            plan.history_push(rows[:, :100])  # neither n_win nor row_length wide
        plan.set_history(6, "u16", LO, HI)  # re-enable: empty, the new shape
        assert plan.history_shape() == (6, 128, "u16") and plan.history_state() == (0, 0)
        with pytest.raises(ValueError):
            plan.history_rows(0, 1)
        plan.history_push(rows)
        same_bits(plan.history_rows(0, 4), hr.stored(rows, "u16", LO, HI), "after the re-enable")
        plan.set_history(0)
        for call in off_calls:
            with pytest.raises(ValueError):
                call()


# ---------------------------------------------------------------- the facade
def test_facade():
    from pypanadapter_amd import History
    rows = np.random.default_rng(51).uniform(-160.0, -40.0, (9, 51)).astype(np.float32)
    hist = History(6, "u8", LO, HI, colormap="Matrix")
    with pytest.raises(AttributeError):
        hist.view(0, 1, 10)
    hist.levels(LO, HI)
    hist.update(rows[:5])
    hist.update(rows[5])
    kept = hr.stored(rows[:6], "u8", LO, HI)
    assert hist.state == (6, 0) and hist.levels() == (LO, HI) and hist.latest(2, 2) == 2
    same_bits(hist.rows(0, 6), kept, "rows")
    geo = (1, 51, 10)
    got = hist.view(hist.latest(2, 2), 2, 10, 2, "min", 1)
    same(got, hr.ref_view(kept, 0, 51, 2, 2, geo, "min", 2), "view")
    rgba = hist.render(hist.latest(3, 3), 3, 10, 3, "min", 1)
    assert rgba.shape == (3, 10, 4) and not rgba[0, :, 3].any() and (rgba[1:, :, 3] == 255).all()
    hist.update(rows[6:])
    assert hist.state == (9, 3) and hist.latest(3) == 6
    same_bits(hist.rows(3, 6), hr.stored(rows[3:], "u8", LO, HI), "after the wrap")
    f = hist.frequencies(10, 2.4e6, 64, 1, col0=1)
    cols = (np.arange(51) - 51 // 2) * (2.4e6 / 64)
    e = vr.edges(1, 51, 10)
    np.testing.assert_allclose(f, [cols[e[i]:e[i + 1]].mean() for i in range(10)], rtol=0, atol=1e-6)
    hist.reset()
    assert hist.state == (0, 0)
    hist.update(rows[:, :20])  # a new width rebuilds the plan and starts empty
    assert hist.state == (9, 3) and hist.view(3, 6, 5).shape == (6, 5)
    hist.close()
