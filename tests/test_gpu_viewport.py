"""GPU checks of the display viewport (zfft_plan_viewport: pushed rows reduced on the device to a
pixel grid, a bucket of columns per pixel and rows_per_line rows per line) against
viewport_ref, the rule of include/zfft.h in numpy (pinned on the CPU by test_viewport_host.py).
MAX and MIN must equal the float32 reference bit for bit (-0.0 and 0.0 compare equal, as the
rule leaves them).  MEAN is held to conftest.assert_row_close, the project's row gate, against
the float64 rule: 1e-3 dB within 100 dB of a line's peak and 1e-5 of the peak amplitude.  The
margin is derived, not measured: the device adds at most four float32 terms before every sum
goes on in float64, so its error is that of 10^(v/20) in float32 (an argument rounding of
1.3e-6 relative at -160 dB, 1.1e-5 dB, plus the function's own ulp); a whole sequential float32
chain of 4096 x 8 values in numpy stays within 2.7e-4 dB.
Worst figures seen on an MI355X (printed by every MEAN check, kept in profiles/viewport/README.md):
max |ddB| 1.07e-5, max |d amp| / peak 3.7e-7 on the synthetic rows; 3.2e-5 and 6.9e-7 against the
float64 Welch row, the float32 lines' own error included."""
import ctypes
import functools

import numpy as np
import pytest

import viewport_ref as vr
import welch_average_ref as war
from conftest import assert_row_close, row_errors

pytestmark = pytest.mark.gpu
FS = war.FS
LINES, SPLIT = 1, 2
WORST = [0.0, 0.0]


def _kind(plan):
    hook = plan.lib.zfft__plan_view_form
    hook.argtypes, hook.restype = [ctypes.c_void_p], ctypes.c_int
    return hook(plan._plan)


def same(got, ref, what=""):
    """Equal as float32 values, NaN in the same places (-0.0 == 0.0)."""
    np.testing.assert_array_equal(np.asarray(got), np.asarray(ref, dtype=np.float32), err_msg=what)


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
        print(f"viewport mean {what} line {i}: max|ddB|={ddb:.3e} max|damp|={damp:.3e} "
              f"(worst so far {WORST[0]:.3e} {WORST[1]:.3e})")
        assert_row_close(a[ok], b[ok], f"{what} line {i}")


def compare(det, got, ref, what=""):
    (mean_close if det == "mean" else same)(got, ref, what)


# name: (n_fft, n_win, in_dtype, (col0, col1, width), rows_per_line, rows, height)
GEOMETRIES = {
    "identity": (64, 64, "complex64", (0, 64, 64), 1, 5, 8),
    "short_real_rows": (1024, 301, "f32", (5, 150, 7), 2, 5, 4),
    "one_pixel": (512, 512, "complex64", (0, 512, 1), 3, 7, 4),
    "display_8192_to_1920": (8192, 8192, "complex64", (0, 8192, 1920), 1, 3, 4),
    "tile_seam": (1024, 1024, "complex64", (3, 1003, 300), 2, 6, 4),       # tiles of 64 pixels: edge 216
    "wide_buckets": (1024, 1024, "complex64", (0, 1024, 3), 1, 2, 2),      # 342 columns a pixel: folded
    "four_waves_a_group": (128, 128, "complex64", (0, 128, 32), 20, 70, 4),
}


@functools.lru_cache(maxsize=None)
def _rows(name, inf):
    """Seeded uniform rows over -160 .. -40 with the specials planted and every column outside the
    window (the tail beyond the row length too) poisoned."""
    N, W, dtype, geo, m, count, _ = GEOMETRIES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    rows = rng.uniform(-160.0, -40.0, (count, W)).astype(np.float32)
    assert vr.plant_specials(rows, geo, m, inf=inf) >= 1
    n = 151 if dtype == "f32" else W
    vr.poison_outside(rows, n, geo)
    rows.setflags(write=False)
    return rows, n


def _check_state(plan, det, lines, pend, height, scroll=1, holds=None, what=""):
    """Image, traces and counters of the plan against the reference lines pushed so far."""
    compare(det, plan.viewport_image(), vr.ref_image(lines, height, scroll), what + " image")
    last, mx, mn = plan.viewport_traces()
    rl, rmx, rmn = vr.ref_holds(lines) if holds is None else holds
    compare(det, last, rl, what + " last")
    compare(det, mx, rmx, what + " max_hold")
    compare(det, mn, rmn, what + " min_hold")


# ---------------------------------------------------------------- 1 and 5. synthetic rows
@pytest.mark.parametrize("det", vr.DETECTORS)
@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_synthetic_rows(name, det):
    from pypanadapter_amd import ZoomFFT
    N, W, dtype, geo, m, count, H = GEOMETRIES[name]
    rows, n = _rows(name, det != "mean")
    with ZoomFFT(N, 1, FS, n_win=W, in_dtype=dtype) as plan:
        assert plan.row_length == n
        plan.set_viewport(H, geo[2], geo[0], geo[1], det, m)
        assert plan.viewport_shape() == (H, geo[2])
        assert np.isnan(plan.viewport_image()).all() and all(np.isnan(t).all() for t in plan.viewport_traces())
        plan.viewport_push(rows)
        lines, pend = vr.ref_lines(rows, n, geo, det, m)
        assert plan.viewport_state() == (count, count // m, count % m) and pend[0] == count % m
        assert _kind(plan) == LINES and len(lines) == count // m >= 1
        _check_state(plan, det, lines, pend, H, what=name)
        if len(lines) < H:
            assert np.isnan(plan.viewport_image()[:H - len(lines)]).all()
        if dtype == "f32":  # cropped rows (as rows() returns them) are padded on the host
            plan.viewport_reset()
            plan.viewport_push(rows[:, :n])
            _check_state(plan, det, lines, pend, H, what=name + " cropped")


# ---------------------------------------------------------------- 2. groups across pushes
@functools.lru_cache(maxsize=None)
def _group_rows():
    geo = (4, 124, 30)
    rows = np.random.default_rng(25).uniform(-160.0, -40.0, (25, 128)).astype(np.float32)
    vr.plant_specials(rows, geo, 5, inf=False)
    vr.poison_outside(rows, 128, geo)
    rows.setflags(write=False)
    return rows, geo


@pytest.mark.parametrize("det", vr.DETECTORS)
def test_groups_across_pushes(det):
    from pypanadapter_amd import ZoomFFT
    rows, geo = _group_rows()
    ref, _ = vr.ref_lines(rows, 128, geo, det, 5)
    with ZoomFFT(128, 1, FS, n_win=128) as plan:
        plan.set_timing(True)
        plan.set_viewport(8, 30, geo[0], geo[1], det, 5)
        plan.viewport_push(rows)
        assert plan.launch_names() == ["view_lines", "view_finish"] and len(plan.timings()) == 2
        whole = plan.viewport_image()
        assert plan.viewport_state() == (25, 5, 0)
        compare(det, whole, vr.ref_image(ref, 8, 1), "one push")
        plan.viewport_reset()
        at = 0
        for cnt, lines, pend in ((1, 0, 1), (3, 0, 4), (7, 2, 1), (4, 3, 0), (10, 5, 0)):
            plan.viewport_push(rows[at:at + cnt])
            at += cnt
            assert plan.viewport_state() == (at, lines, pend)
            if lines == 0:  # a push that completes no line leaves image and traces empty
                assert np.isnan(plan.viewport_image()).all() and np.isnan(plan.viewport_traces()[0]).all()
        parts = plan.viewport_image()
        if det == "mean":
            mean_close(parts[3:], ref, "five pushes")
        else:
            assert parts.tobytes() == whole.tobytes() or np.array_equal(parts, whole, equal_nan=True)
            same(parts, vr.ref_image(ref, 8, 1), "five pushes")
        _check_state(plan, det, ref, None, 8, what="five pushes")


# ---------------------------------------------------------------- 3. more lines than the image
@pytest.mark.parametrize("det", vr.DETECTORS)
def test_more_lines_than_the_image(det):
    from pypanadapter_amd import ZoomFFT
    geo = (0, 200, 50)
    rows = np.random.default_rng(37).uniform(-160.0, -40.0, (37, 256)).astype(np.float32)
    vr.poison_outside(rows, 256, geo)
    ref, pend = vr.ref_lines(rows, 256, geo, det, 2)
    for scroll in (1, -1):
        with ZoomFFT(256, 1, FS, n_win=256, scroll=scroll) as plan:
            plan.set_viewport(4, 50, 0, 200, det, 2)
            plan.viewport_push(rows)
            assert plan.viewport_state() == (37, 18, 1) and len(ref) == 18 and pend[0] == 1
            _check_state(plan, det, ref, pend, 4, scroll, what=f"scroll {scroll}")
            img = plan.viewport_image()
            compare(det, img[3 if scroll > 0 else 0], ref[17], "newest")
            compare(det, img[0 if scroll > 0 else 3], ref[14], "oldest kept")


# ---------------------------------------------------------------- 4. a group split over workgroups
@functools.lru_cache(maxsize=None)
def _split_rows():
    geo = (0, 128, 32)
    rows = np.random.default_rng(3000).uniform(-160.0, -40.0, (9000, 128)).astype(np.float32)
    rows[17, 5] = rows[4000, 64] = np.nan
    rows.setflags(write=False)
    return rows, geo


@pytest.mark.parametrize("det", ["max", "mean"])
def test_group_split_over_workgroups(det):
    from pypanadapter_amd import ZoomFFT
    rows, geo = _split_rows()
    ref, _ = vr.ref_lines(rows, 128, geo, det, 3000)
    assert len(ref) == 3
    with ZoomFFT(128, 1, FS, n_win=128) as plan:
        plan.set_timing(True)
        plan.set_viewport(4, 32, 0, 128, det, 3000)
        plan.viewport_push(rows[:7000])
        assert _kind(plan) == SPLIT and plan.launch_names() == ["view_lines", "view_finish"]
        assert plan.viewport_state() == (7000, 2, 1000)
        _check_state(plan, det, ref[:2], None, 4, what="7000 rows")
        plan.viewport_push(rows[7000:8000])
        assert _kind(plan) == SPLIT and plan.viewport_state() == (8000, 2, 2000)
        _check_state(plan, det, ref[:2], None, 4, what="8000 rows")
        plan.viewport_push(rows[8000:])  # the pending 2000 rows were the reference's: line 2 tells
        assert plan.viewport_state() == (9000, 3, 0)
        _check_state(plan, det, ref, None, 4, what="9000 rows")


# ---------------------------------------------------------------- 6. against the Welch reference
WELCH = {"dif1024_nseg17": (1024, 1, 1024, 9216, 5, 17), "stockham_n512_zoom2": (512, 2, 256, 8192, 2, 15)}


@pytest.mark.parametrize("name", sorted(WELCH))
def test_against_the_welch_reference(oracle_lib, name):
    """The lines of a plan with segments_per_line = 1 are one Welch segment each: their MEAN over
    a frame (width = span = n, rows_per_line = the frame's lines) is the frame's Welch row, their
    MAX its average="max" row."""
    from pypanadapter_amd import ZoomFFT
    N, zoom, W, L, F, R = WELCH[name]
    x = war.burst_frames(F, L, N, zoom, W, 9100)
    with ZoomFFT(N, zoom, FS, n_win=W) as whole:
        plain = whole.rows(x)
    with ZoomFFT(N, zoom, FS, n_win=W, segments_per_line=1) as plan:
        assert plan.lines(L) == R
        lines = plan.rows(x).reshape(F * R, W)
        for det in ("mean", "max"):
            plan.set_viewport(8, W, 0, W, det, R)
            plan.viewport_push(lines)
            assert plan.viewport_state() == (F * R, F, 0) and _kind(plan) == LINES
            img = plan.viewport_image()[8 - F:]
            for f in range(F):
                ref = war.ref_row(x[f], FS, N, zoom, W, det)
                ddb, damp = row_errors(img[f], ref)
                print(f"viewport {name} {det} frame {f}: max|ddB|={ddb:.3e} max|damp|={damp:.3e}")
                assert_row_close(img[f], ref, f"{name} {det} frame {f} vs float64")
                if det == "mean":
                    assert_row_close(img[f], plain[f], f"{name} frame {f} vs the whole-frame row")


# ---------------------------------------------------------------- 7. order, reset, lifecycle
def test_scroll_reset_and_hold_reset():
    from pypanadapter_amd import ZoomFFT
    geo = (0, 64, 16)
    rows = np.random.default_rng(7).uniform(-160.0, -40.0, (6, 64)).astype(np.float32)
    ref, _ = vr.ref_lines(rows, 64, geo, "max", 1)
    with ZoomFFT(64, 1, FS, n_win=64, scroll=-1) as plan:
        plan.set_viewport(4, 16)
        plan.viewport_push(rows[:3])
        img = plan.viewport_image()
        same(img[0], ref[2], "newest at row 0")
        same(img, vr.ref_image(ref[:3], 4, -1))
        plan.viewport_hold_reset()  # the holds only
        last, mx, mn = plan.viewport_traces()
        same(last, ref[2])
        assert np.isnan(mx).all() and np.isnan(mn).all() and plan.viewport_state() == (3, 3, 0)
        same(plan.viewport_image(), img)
        plan.viewport_push(rows[3:4])
        _check_state(plan, "max", ref[:4], None, 4, -1, holds=vr.ref_holds(ref[3:4]))
        plan.waterfall_reset(1)  # cfg.scroll changes; the viewport reads it at its next reset
        plan.viewport_push(rows[4:5])
        same(plan.viewport_image()[0], ref[4], "still scrolling down")
        plan.viewport_reset()
        assert plan.viewport_state() == (0, 0, 0) and np.isnan(plan.viewport_image()).all()
        assert all(np.isnan(t).all() for t in plan.viewport_traces())
        plan.viewport_push(rows[:2])
        same(plan.viewport_image(), vr.ref_image(ref[:2], 4, 1), "scroll +1 after the reset")
        # a reset drops the pending group too
        plan.set_viewport(4, 16, rows_per_line=3)
        plan.viewport_push(rows[:2])
        assert plan.viewport_state() == (2, 0, 2)
        plan.viewport_reset()
        plan.viewport_push(rows[3:6])
        same(plan.viewport_image()[3], vr.ref_lines(rows[3:6], 64, geo, "max", 3)[0][0])


def test_reenable_validation_and_off():
    from pypanadapter_amd import ZoomFFT, _lib
    rows = np.random.default_rng(8).uniform(-160.0, -40.0, (4, 8192)).astype(np.float32)
    with ZoomFFT(8192, 1, FS, n_win=8192) as plan:
        lib, h = plan.lib, plan._plan
        hh, ww = ctypes.c_int32(-1), ctypes.c_int32(-1)
        assert lib.zfft_viewport_shape(h, ctypes.byref(hh), ctypes.byref(ww)) == _lib.ZFFT_EINVAL
        assert (hh.value, ww.value) == (0, 0)
        off_calls = (plan.viewport_image, plan.viewport_traces, plan.viewport_state, plan.viewport_reset,
                     plan.viewport_hold_reset, plan.viewport_render, lambda: plan.viewport_push(rows),
                     lambda: plan.viewport_push_device(8, 1), lambda: plan.viewport_render_device(8),
                     lambda: plan.viewport_push_render(rows[0]), plan.viewport_shape)
        for call in off_calls:
            with pytest.raises(ValueError):
                call()
        # (height, width, col0, col1, detector, rows_per_line)
        for bad in ((-1, 16, 0, 64, 0, 1), (8193, 16, 0, 64, 0, 1), (4, 0, 0, 64, 0, 1), (4, 65, 0, 64, 0, 1),
                    (4, 16, -1, 64, 0, 1), (4, 16, 64, 64, 0, 1), (4, 16, 70, 64, 0, 1), (4, 16, 0, 8193, 0, 1),
                    (8192, 4097, 0, 8192, 0, 1), (4, 16, 0, 64, 3, 1), (4, 16, 0, 64, -1, 1), (4, 16, 0, 64, 0, 0),
                    (4, 16, 0, 64, 0, 65537)):
            assert lib.zfft_plan_viewport(h, *bad) == _lib.ZFFT_EINVAL, bad
        with pytest.raises(ValueError):
            plan.set_viewport(4, 16, detector="median")
        assert lib.zfft_plan_viewport(h, 8192, 4096, 0, 8192, 2, 65536) == _lib.ZFFT_OK  # the limits themselves
        plan.set_viewport(4, 16, 0, 64)
        plan.viewport_push(rows[:3])
        plan.set_viewport(2, 100, 100, 8000, "min", 2)  # another geometry: empty, the new shape
        assert plan.viewport_shape() == (2, 100) and plan.viewport_state() == (0, 0, 0)
        assert np.isnan(plan.viewport_image()).all() and np.isnan(plan.viewport_traces()[1]).all()
        plan.viewport_push(rows)
        ref, _ = vr.ref_lines(rows, 8192, (100, 8000, 100), "min", 2)
        _check_state(plan, "min", ref, None, 2)
        with pytest.raises(ValueError):
            plan.viewport_push(rows[:, :100])  # neither n_win nor row_length wide
        plan.set_viewport(0, 0)
        for call in off_calls:
            with pytest.raises(ValueError):
                call()


# ---------------------------------------------------------------- 8. render and the device path
def _render_ref(plan, img, cmap):
    from oracle import render as orender
    ref = orender.render(np.nan_to_num(img.astype(np.float64), nan=0.0), orender.lookup_table(cmap),
                         plan.waterfall_levels())
    ref[np.isnan(img)] = (*orender.lookup_table(cmap)[0][:3], 0)
    return ref


def test_render_on_a_plan_too_narrow_for_the_ring():
    from pypanadapter_amd import ZoomFFT, pinned_empty
    rows = np.random.default_rng(32).uniform(-230.0, -110.0, (3, 32)).astype(np.float32)
    rows[1, 7] = np.nan
    with ZoomFFT(32, 1, FS, n_win=32) as plan:
        with pytest.raises(ValueError):
            plan.waterfall_push(rows[0])  # n_win 32: no reference ring
        plan.set_viewport(5, 32)
        plan.waterfall_colormap("Tropical")
        plan.waterfall_levels(-200.0, -130.0)
        plan.viewport_push(rows[:2])
        img = plan.viewport_image()
        assert np.isnan(img[:3]).all() and np.isnan(img[4, 7])
        rgba = plan.viewport_render()
        assert rgba.shape == (5, 32, 4) and rgba.dtype == np.uint8
        np.testing.assert_array_equal(rgba, _render_ref(plan, img, "Tropical"))
        assert not rgba[:3, :, 3].any() and rgba[4, 7, 3] == 0 and (rgba[3, :, 3] == 255).all()
        # push + render in one round trip equals push, then render: pageable, page-locked, engine-owned
        with ZoomFFT(32, 1, FS, n_win=32) as two:
            two.set_viewport(5, 32)
            two.waterfall_colormap("Tropical")
            two.waterfall_levels(-200.0, -130.0)
            two.viewport_push(rows[:2])
            two.viewport_push(rows[2])
            want = two.viewport_render(np.empty((5, 32, 4), np.uint8))
        for out in (np.empty((5, 32, 4), np.uint8), pinned_empty((5, 32, 4), np.uint8), None):
            plan.viewport_reset()
            plan.viewport_push(rows[:2])
            got = plan.viewport_push_render(rows[2], out)
            np.testing.assert_array_equal(got, want)
            np.testing.assert_array_equal(plan.viewport_push_render(None, out), want)
        with pytest.raises(ValueError):
            plan.viewport_render(np.empty((5, 32, 3), np.uint8))


def test_device_rows_pushed_on_the_same_stream():
    """process_device into a torch buffer, then viewport_push_device and viewport_render_device on
    the same stream: image and pixels equal the host path on the rows copied back."""
    import torch
    from pypanadapter_amd import ZoomFFT
    N, zoom, W, L, F, R = WELCH["stockham_n512_zoom2"]
    x = war.burst_frames(F, L, N, zoom, W, 9100)
    dev = torch.device("cuda:0")
    xd = torch.from_numpy(np.array(x).view(np.float32).reshape(F, L, 2)).to(dev)
    geo = (10, 250, 60)
    with ZoomFFT(N, zoom, FS, n_win=W, segments_per_line=1) as plan:
        plan.set_timing(True)
        plan.set_viewport(8, 60, geo[0], geo[1], "max", 4)
        rows = torch.empty((F * R, W), device=dev, dtype=torch.float32)
        rgba = torch.empty((8, 60, 4), device=dev, dtype=torch.uint8)
        st = torch.cuda.current_stream().cuda_stream
        plan.process_device(xd.data_ptr(), L, F, rows.data_ptr(), st)
        plan.viewport_push_device(rows.data_ptr(), F * R, st)
        plan.viewport_render_device(rgba.data_ptr(), st)
        names = plan.launch_names()
        img = plan.viewport_image()
        torch.cuda.synchronize()
        host = rows.cpu().numpy()
        assert names == ["view_lines", "view_finish"] and plan.viewport_state() == (30, 7, 2)
        ref, _ = vr.ref_lines(host, W, geo, "max", 4)
        same(img, vr.ref_image(ref, 8, 1))
        assert np.isfinite(img[1:]).all()
        np.testing.assert_array_equal(rgba.cpu().numpy(), plan.viewport_render())
        plan.viewport_reset()
        plan.viewport_push(host)
        assert plan.viewport_image().tobytes() == img.tobytes()
        # one aligned group in one workgroup per tile is a single launch
        plan.set_viewport(8, 60, geo[0], geo[1], "max", 1)
        plan.viewport_push(host[0])
        assert plan.launch_names() == ["view_lines"] and len(plan.timings()) == 1
        same(plan.viewport_traces()[1], vr.ref_lines(host[:1], W, geo, "max", 1)[0][0])


# ---------------------------------------------------------------- the facade
def test_facade():
    from pypanadapter_amd import Viewport
    rows = np.random.default_rng(51).uniform(-230.0, -110.0, (9, 51)).astype(np.float32)
    view = Viewport(4, 10, detector="min", rows_per_line=2, col0=1, col1=51, colormap="Matrix")
    with pytest.raises(AttributeError):
        view.image()
    view.levels(-200.0, -130.0)
    view.update(rows[:5])
    view.update(rows[5])
    ref, _ = vr.ref_lines(rows[:6], 51, (1, 51, 10), "min", 2)
    same(view.image(), vr.ref_image(ref, 4, 1))
    assert view.state == (6, 3, 0) and view.levels() == (-200.0, -130.0)
    last, mx, mn = view.traces()
    same(mn, vr.ref_holds(ref)[2])
    rgba = view.render()
    assert rgba.shape == (4, 10, 4) and not rgba[0, :, 3].any() and (rgba[1:, :, 3] == 255).all()
    np.testing.assert_array_equal(rgba, _render_ref(view._plan, view.image(), "Matrix"))
    # pixel x is the mean of its bucket's columns in Detector.frequencies' mapping
    f = view.frequencies(2.4e6, 64, 1)
    cols = (np.arange(51) - 51 // 2) * (2.4e6 / 64)
    e = vr.edges(1, 51, 10)
    np.testing.assert_allclose(f, [cols[e[i]:e[i + 1]].mean() for i in range(10)], rtol=0, atol=1e-6)
    view.hold_reset()
    assert np.isnan(view.traces()[1]).all()
    view.reset()
    assert view.state == (0, 0, 0) and np.isnan(view.image()).all()
    with pytest.raises(ValueError):
        view.update(rows[:, :20])  # a new width rebuilds the plan: the window [1, 51) no longer fits
    wide = Viewport(2, 5)
    wide.update(rows)
    wide.update(rows[:, :20])      # without a fixed col1 the whole of the new width is shown
    same(wide.image()[1], vr.ref_lines(rows[-1:, :20], 20, (0, 20, 5), "max", 1)[0][0])
    assert wide.state == (9, 9, 0)
    wide.close()
    view.close()
