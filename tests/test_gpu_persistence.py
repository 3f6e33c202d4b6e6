"""GPU checks of the persistence spectrum (zfft_plan_persistence: a per-column histogram of the
pushed rows' levels, accumulated on the device) against persistence_ref.ref_hist, the binning
rule of include/zfft.h in numpy float32 (pinned on the CPU by test_persistence_host.py).  The
device's table must equal it as integers: the rule is two float32 roundings and a truncation,
and integer sums do not depend on the order.  Only the comparison against the float64 Welch
reference (test 5) has a bound, the number of reference values within twice the row gate of a
level edge."""
import ctypes
import functools

import numpy as np
import pytest

import persistence_ref as pr
import welch_average_ref as war
import welch_lines_ref as wlr

pytestmark = pytest.mark.gpu
FS = war.FS

# name: (N, zoom, W, L, frames, g) -- the shapes of test_gpu_welch_lines.py's cases of these names
SHAPES = {
    "stockham_n64_groups_4_4_3": (64, 1, 64, 64 + 32 * 10, 2, 1),
    "stockham_n512_zoom2": (512, 2, 256, 8192, 2, 1),
    "dif1024_nseg17": (1024, 1, 1024, 9216, 5, 1),
    "dif4096_pruned_zoom8": (4096, 8, 512, 98304, 1, 2),
}
SEED = 9100


@functools.lru_cache(maxsize=None)
def _frames(name):
    N, zoom, W, L, F, _ = SHAPES[name]
    x = war.burst_frames(F, L, N, zoom, W, SEED)
    x.setflags(write=False)
    return x


def _slices(plan):
    hook = plan.lib.zfft__plan_persist_slices
    hook.argtypes, hook.restype = [ctypes.c_void_p], ctypes.c_int
    return hook(plan._plan)


def _synthetic(count, n_win, row_len, levels, db_min, db_max, seed):
    """Seeded rows over a little more than the range (every column, the unread tail too), with
    the binning's edge values planted at the head."""
    rng = np.random.default_rng(seed)
    span = db_max - db_min
    rows = rng.uniform(db_min - 0.1 * span, db_max + 0.1 * span, (count, n_win)).astype(np.float32)
    assert pr.plant_edges(rows, levels, db_min, db_max, row_len) >= min(levels + 7, count * row_len)
    return rows


# ---------------------------------------------------------------- 1. exact, synthetic rows
WIDTHS = {"w64_one_block": (64, 64, "complex64"), "w50_masked_block": (64, 50, "complex64"),
          "w200_masked_tail": (256, 200, "complex64"), "w512_cfg2": (512, 512, "complex64"),
          "w301_real_short_rows": (1024, 301, "f32")}


@pytest.mark.parametrize("levels", [2, 5, 256])
@pytest.mark.parametrize("width", sorted(WIDTHS))
def test_exact_on_synthetic_rows(width, levels):
    from pypanadapter_amd import ZoomFFT
    N, W, dtype = WIDTHS[width]
    count, lo, hi = 37, -100.0, -60.0
    with ZoomFFT(N, 1, FS, n_win=W, in_dtype=dtype) as plan:
        n = plan.row_length
        assert (n < W) == (dtype == "f32") and n == (151 if dtype == "f32" else W)
        rows = _synthetic(count, W, n, levels, lo, hi, 100 * W + levels)
        plan.set_persistence(levels, lo, hi)
        assert plan.persistence_shape() == (levels, W)
        plan.persistence_push(rows)
        hist, seen = plan.persistence()
        ref = pr.ref_hist(rows, levels, lo, hi, n)
        assert hist.dtype == np.uint32 and hist.shape == (levels, W) and seen == count
        np.testing.assert_array_equal(hist, ref)
        assert not hist[:, n:].any() and hist.sum() > count * n // 2
        # cropped rows (as rows() returns them) are padded on the host: the same table again
        plan.persistence_reset()
        plan.persistence_push(rows[:, :n])
        np.testing.assert_array_equal(plan.persistence()[0], ref)


# ---------------------------------------------------------------- 2. many rows
@functools.lru_cache(maxsize=None)
def _concentrated():
    """20,000 x 128 rows over 256 levels of 0.5 dB: 90 % of each column's values fall in three
    adjacent levels around the column's own centre (the noise floor), the rest anywhere."""
    count, W, levels, lo, hi = 20000, 128, 256, -130.0, -2.0
    rng = np.random.default_rng(4242)
    centre = rng.integers(1, levels - 1, W)
    near = lo + (centre[None, :] - 1 + 3.0 * rng.random((count, W))) * 0.5
    wide = rng.uniform(lo - 5.0, hi + 5.0, (count, W))
    rows = np.where(rng.random((count, W)) < 0.9, near, wide).astype(np.float32)
    ref = pr.ref_hist(rows, levels, lo, hi, W)
    top3 = np.sort(ref, axis=0)[-3:].sum(axis=0)
    assert np.all(top3 >= 0.88 * count)
    rows.setflags(write=False)
    ref.setflags(write=False)
    return rows, ref, (levels, lo, hi)


def test_many_concentrated_rows_take_several_slices():
    from pypanadapter_amd import ZoomFFT
    rows, ref, (levels, lo, hi) = _concentrated()
    with ZoomFFT(128, 1, FS, n_win=128) as plan:
        plan.set_timing(True)
        plan.set_persistence(levels, lo, hi)
        plan.persistence_push(rows)
        assert _slices(plan) > 1
        assert plan.launch_names() == ["persist_hist"] and len(plan.timings()) == 1
        hist, seen = plan.persistence()
        assert seen == len(rows)
        np.testing.assert_array_equal(hist, ref)


def test_single_row_pushes_then_the_rest_give_the_same_table():
    from pypanadapter_amd import ZoomFFT
    rows, ref, (levels, lo, hi) = _concentrated()
    with ZoomFFT(128, 1, FS, n_win=128) as plan:
        plan.set_persistence(levels, lo, hi)
        for r in rows[:300]:
            plan.persistence_push(r)
        assert _slices(plan) == 1
        plan.persistence_push(rows[300:])
        hist, seen = plan.persistence()
        assert seen == len(rows)
        np.testing.assert_array_equal(hist, ref)


# ---------------------------------------------------------------- 3. accumulation, decay, reset
def test_accumulation_decay_reset_and_off():
    from pypanadapter_amd import ZoomFFT, _lib
    W, lo, hi = 64, -100.0, -60.0
    a = _synthetic(37, W, W, 5, lo, hi, 1)
    b = _synthetic(11, W, W, 5, lo, hi, 2)
    ra, rb = pr.ref_hist(a, 5, lo, hi, W), pr.ref_hist(b, 5, lo, hi, W)
    with ZoomFFT(64, 1, FS, n_win=W) as plan:
        with pytest.raises(ValueError):  # off by default
            plan.persistence()
        lv, cols = ctypes.c_int32(-1), ctypes.c_int32(-1)
        rc = plan.lib.zfft_persistence_shape(plan._plan, ctypes.byref(lv), ctypes.byref(cols))
        assert rc == _lib.ZFFT_EINVAL and lv.value == 0
        for bad in ((1, lo, hi), (257, lo, hi), (-1, lo, hi), (5, hi, lo), (5, lo, lo),
                    (5, float("nan"), hi), (5, lo, float("inf"))):
            with pytest.raises(ValueError):
                plan.set_persistence(*bad)
        plan.set_persistence(5, lo, hi)
        plan.persistence_push(a)
        plan.persistence_push(b)
        hist, seen = plan.persistence()
        np.testing.assert_array_equal(hist, ra + rb)
        assert seen == 48
        np.testing.assert_array_equal(plan.persistence_density(), (ra + rb) / 48.0)
        plan.persistence_decay(1.0)
        np.testing.assert_array_equal(plan.persistence()[0], ra + rb)
        plan.persistence_decay(0.5)
        hist, seen = plan.persistence()
        np.testing.assert_array_equal(hist, (ra + rb) // 2)
        assert seen == 24
        for bad in (-0.1, 1.5, float("nan")):
            with pytest.raises(ValueError):
                plan.persistence_decay(bad)
        plan.persistence_decay(0.0)
        hist, seen = plan.persistence()
        assert not hist.any() and seen == 0
        plan.persistence_push(a)
        plan.persistence_reset()
        hist, seen = plan.persistence()
        assert not hist.any() and seen == 0
        assert plan.persistence_density().shape == (5, W)
        plan.persistence_push(a)
        plan.set_persistence(8, lo, hi)  # re-enabled with other parameters: zeros, the new shape
        hist, seen = plan.persistence()
        assert hist.shape == (8, W) and not hist.any() and seen == 0
        plan.persistence_push(b)
        np.testing.assert_array_equal(plan.persistence()[0], pr.ref_hist(b, 8, lo, hi, W))
        plan.set_persistence(0)
        for call in (plan.persistence, plan.persistence_reset, lambda: plan.persistence_decay(0.5),
                     lambda: plan.persistence_push(a), lambda: plan.persistence_push_device(8, 1)):
            with pytest.raises(ValueError):
                call()


# ---------------------------------------------------------------- 4. behind the real path
@pytest.mark.parametrize("name", ["dif1024_nseg17", "stockham_n512_zoom2"])
def test_device_rows_pushed_on_the_same_stream(name):
    """process_device into a torch buffer, then persistence_push_device of that buffer on the same
    stream: the table is ref_hist of the rows copied back, and the rows are bytewise those of a
    plan with persistence off."""
    import torch
    from pypanadapter_amd import ZoomFFT
    N, zoom, W, L, F, g = SHAPES[name]
    x = _frames(name)
    dev = torch.device("cuda:0")
    xd = torch.from_numpy(np.array(x).view(np.float32).reshape(F, L, 2)).to(dev)  # (a writable copy)
    with ZoomFFT(N, zoom, FS, n_win=W, segments_per_line=g) as off:
        plain = off.rows(x).reshape(-1, W)
    assert len(plain) == {"dif1024_nseg17": 85, "stockham_n512_zoom2": 30}[name]
    hi = float(np.ceil(plain[np.isfinite(plain)].max())) + 2.0
    lo, levels = hi - 96.0, 96
    with ZoomFFT(N, zoom, FS, n_win=W, segments_per_line=g) as plan:
        R = plan.lines(L)
        plan.set_persistence(levels, lo, hi)
        rows = torch.empty((F * R, W), device=dev, dtype=torch.float32)
        st = torch.cuda.current_stream().cuda_stream
        plan.process_device(xd.data_ptr(), L, F, rows.data_ptr(), st)
        plan.persistence_push_device(rows.data_ptr(), F * R, st)
        hist, seen = plan.persistence()
        torch.cuda.synchronize()
        host = rows.cpu().numpy()
    assert seen == F * R
    assert host.tobytes() == plain.tobytes()
    ref = pr.ref_hist(host, levels, lo, hi, W)
    np.testing.assert_array_equal(hist, ref)
    assert ref.sum() >= 0.1 * host.size


# ---------------------------------------------------------------- 5. against the float64 reference
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_against_the_float64_reference(oracle_lib, name):
    """The table of the device's fp32 lines against ref_hist of welch_lines_ref.ref_lines: 96 levels
    of 1 dB ending 2 dB above the largest reference value, so every counted value lies within
    100 dB of its line's peak, where the row gate bounds the dB error by 1e-3.  A value may then
    change its level only when the reference lies within 2e-3 dB of an edge: half the summed
    absolute difference of the tables is at most the number n_edge of such reference values."""
    from pypanadapter_amd import ZoomFFT
    N, zoom, W, L, F, g = SHAPES[name]
    x = _frames(name)
    ref_rows = np.concatenate([wlr.ref_lines(x[f], FS, N, zoom, W, g, "mean") for f in range(F)])
    assert ref_rows.size == {"stockham_n64_groups_4_4_3": 1408, "stockham_n512_zoom2": 7680,
                             "dif1024_nseg17": 87040, "dif4096_pruned_zoom8": 1536}[name]
    hi = float(np.ceil(ref_rows[np.isfinite(ref_rows)].max())) + 2.0
    lo, levels = hi - 96.0, 96
    ref = pr.ref_hist(ref_rows.astype(np.float32), levels, lo, hi, W)
    # the edges are the integers lo .. hi
    with np.errstate(invalid="ignore"):  # (a zero bin's -inf is near no edge)
        near = (np.abs(ref_rows - np.round(ref_rows)) <= 2e-3) & (ref_rows >= lo - 2e-3) & (ref_rows <= hi + 2e-3)
    n_edge = int(near.sum())
    with ZoomFFT(N, zoom, FS, n_win=W, segments_per_line=g) as plan:
        lines = plan.rows(x).reshape(-1, W)
        assert lines.shape == ref_rows.shape
        plan.set_persistence(levels, lo, hi)
        plan.persistence_push(lines)
        hist, seen = plan.persistence()
    assert seen == len(ref_rows)
    moved = np.abs(hist.astype(np.int64) - ref.astype(np.int64)).sum() / 2.0
    print(f"{name}: n_edge={n_edge} ({n_edge / ref_rows.size:.2%}) moved={moved} "
          f"in range={ref.sum() / ref_rows.size:.1%}")
    assert n_edge <= 0.01 * ref_rows.size
    assert ref.sum() >= 0.1 * ref_rows.size and hist.sum() >= 0.1 * ref_rows.size
    assert moved <= n_edge


# ---------------------------------------------------------------- 6. the facade
def test_facade_takes_psd_lines():
    from pypanadapter_amd import panadapter
    N, zoom, W, L, F, g = SHAPES["stockham_n512_zoom2"]
    x = _frames("stockham_n512_zoom2")[0]
    lines = panadapter.psd_lines(x, FS, N, zoom, g)
    assert lines.shape == (15, W)
    view = panadapter.Persistence(levels=200, db_min=-220.0, db_max=-20.0)
    with pytest.raises(AttributeError):
        view.image()
    view.update(lines)
    ref = pr.ref_hist(lines.astype(np.float32), 200, -220.0, -20.0, W)
    np.testing.assert_array_equal(view.image(), ref)
    assert ref.sum() > 0.9 * lines.size and view.rows_seen == 15
    view.update(lines[0])
    np.testing.assert_array_equal(view.image(), ref + pr.ref_hist(lines[:1].astype(np.float32), 200, -220.0, -20.0, W))
    np.testing.assert_array_equal(view.density(), view.image() / 16.0)
    view.decay(0.5)
    assert view.rows_seen == 8
    view.reset()
    assert not view.image().any() and view.rows_seen == 0
    # a width change rebuilds the plan and starts from zeros; an odd width keeps every column
    narrow = np.random.default_rng(7).uniform(-230.0, -10.0, (9, 51)).astype(np.float32)
    view.update(lines)
    view.update(narrow)
    img = view.image()
    assert img.shape == (200, 51) and view.rows_seen == 9
    np.testing.assert_array_equal(img, pr.ref_hist(narrow, 200, -220.0, -20.0, 51))
    view.close()
