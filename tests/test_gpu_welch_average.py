"""GPU checks of the Welch detectors (zfft_plan_average: mean / median / max over a frame's
segments) against the float64 reference of welch_average_ref.py (pinned on the CPU by
test_welch_average.py), under the project's row gate (conftest.assert_row_close: 1e-3 dB within
100 dB of the row's peak, 1e-5 of the peak amplitude).  The inputs carry a burst in one or two
segments, so the three rows differ by tens of dB and a mode that is ignored fails.  The shapes
are the smallest that reach each Welch kernel family and form, and each way welch_select holds
a column's keys (registers up to 32 segments, LDS up to 256, the scratch itself beyond)."""
import ctypes

import numpy as np
import pytest

import welch_average_ref as war
from conftest import assert_row_close, row_errors
from welch_plan_check import assert_plan_ran

pytestmark = pytest.mark.gpu
FS = war.FS
MODES = ("mean", "median", "max")


def _hooks(plan):
    cap = plan.lib.zfft__plan_average_cap
    cap.argtypes, cap.restype = [ctypes.c_void_p, ctypes.c_int64], ctypes.c_int
    split = plan.lib.zfft__plan_welch_split
    split.argtypes, split.restype = [ctypes.c_void_p], ctypes.c_int
    return cap, split


def _check(rows, x, N, zoom, W, average, what, frames=None):
    rows = np.atleast_2d(rows)
    for f in (range(len(x)) if frames is None else frames):
        ref = war.ref_row(x[f], FS, N, zoom, W, average)
        assert rows[f].shape == ref.shape, (what, rows[f].shape, ref.shape)
        ddb, damp = row_errors(rows[f], ref)
        print(f"{what} {average} frame {f}: max|ddB|={ddb:.3e} max|damp|={damp:.3e}")
        assert_row_close(rows[f], ref, f"{what} {average} frame {f}")


def _sel_len(N, nseg):
    return N + (N // 2) * (nseg - 1)


# name: (N, zoom, W, L, frames, options)
CASES = {
    # Stockham kernel (N < 1024): 400 segments (the long selection loop), and behind zoom 2
    "stockham_n64_400seg": (64, 1, 64, 12832, 1, {}),
    "stockham_n512_zoom2": (512, 2, 256, 8192, 2, {}),
    # in-place DIF, several frames per workgroup (5 frames: a spare frame slot), even / odd nseg
    "dif1024_nseg16": (1024, 1, 1024, 8704, 5, {}),
    "dif1024_nseg17": (1024, 1, 1024, 9216, 5, {}),
    # DIF N = 4096 pruned behind the automatic decimator (PC tiles), and FC in front of N = 1024
    "dif4096_pruned_zoom8": (4096, 8, 512, 98304, 1, {}),
    "dif1024_fc_in_front": (1024, 8, 128, 32768, 16, {"first": "fc_decim"}),
    "dif4096_full": (4096, 1, 4096, 12288, 1, {}),
    # DIF N = 16384 (single prefetch array), pruned and full
    "dif16384_pruned": (16384, 1, 2048, 32768, 1, {}),
    "dif16384_full": (16384, 1, 16384, 32768, 1, {}),
    # the split few-frames form
    "split_1_frame": (1024, 1, 1024, 2560, 1, {"split": True}),
    "split_2_frames": (1024, 1, 1024, 2560, 2, {"split": True}),
    # four-step, pruned (W = N / 8) and full, and forced at N = 4096
    "four_32768_pruned": (32768, 1, 4096, 65536, 2, {"four": True}),
    "four_32768_full": (32768, 1, 32768, 65536, 2, {"four": True}),
    "four_65536_pruned": (65536, 1, 8192, 131072, 2, {"four": True}),
    "four_65536_full": (65536, 1, 65536, 131072, 2, {"four": True}),
    "four_4096_forced": (4096, 1, 512, 12288, 2, {"four": True, "welch": 2}),
    # nseg = 1, 2, 3
    "nseg1": (32, 1, 32, 32, 1, {}),
    "nseg2": (32, 1, 32, 48, 1, {}),
    "nseg3": (32, 1, 32, 64, 1, {}),
    # one-sided rows: real input at zoom 1, even and odd W
    "onesided_even_w": (1024, 1, 1024, 9216, 2, {"real": True}),
    "onesided_odd_w": (1024, 1, 301, 9216, 2, {"real": True}),
    # welch_select's thresholds: registers <= 32 < LDS <= 256 < scratch (even and odd nseg)
    "select_nseg32": (64, 1, 50, _sel_len(64, 32), 2, {}),
    "select_nseg33": (64, 1, 50, _sel_len(64, 33), 2, {}),
    "select_nseg100": (64, 1, 50, _sel_len(64, 100), 2, {}),
    "select_nseg256": (64, 1, 50, _sel_len(64, 256), 2, {}),
    "select_nseg257": (64, 1, 50, _sel_len(64, 257), 2, {}),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_detectors_vs_float64_reference(oracle_lib, name):
    from pypanadapter_amd import ZoomFFT
    N, zoom, W, L, F, opt = CASES[name]
    real = opt.get("real", False)
    x = war.burst_frames(F, L, N, zoom, W, 5000 + 13 * sorted(CASES).index(name), real=real)
    with ZoomFFT(N, zoom, FS, n_win=W, in_dtype="f32" if real else "complex64") as plan:
        _, split = _hooks(plan)
        plan.set_timing(True)
        if "welch" in opt:
            plan.set_welch(opt["welch"])
        splits = {}
        for average in MODES:
            plan.set_average(average)
            rows = plan.rows(x)
            desc = assert_plan_ran(plan, L, F, welch=opt.get("welch", 0))
            assert desc.startswith("four ") == bool(opt.get("four")), desc
            names = plan.launch_names()
            splits[average] = split(plan._plan)
            if average == "mean":
                assert names[-1] == ("welch4" if opt.get("four") else "welch_rows"), names
            else:
                assert names[-2:] == ["welch4_segs" if opt.get("four") else "welch_segs", "welch_select"], names
            if "first" in opt:
                assert names[0] == opt["first"], names
            _check(rows, x, N, zoom, W, average, name)
        if not opt.get("four"):  # the detectors split a frame's segments where mean does
            assert splits["median"] == splits["max"] == splits["mean"], splits
            if opt.get("split"):
                assert splits["mean"] > 1, splits


def test_short_input_branch_all_modes_agree(oracle_lib):
    """L_d = 624 < N: one segment of 624 samples zero-padded to N, so median (bias(1) = 1) and
    max are the mean row; each within the gate of the reference, and of the mean row."""
    from pypanadapter_amd import ZoomFFT
    N, zoom, W, L = 2048, 512, 2048, 319488
    x = war.burst_frames(1, L, N, zoom, W, 5900)
    rows = {}
    with ZoomFFT(N, zoom, FS, n_win=W) as plan:
        plan.set_timing(True)
        for average in MODES:
            plan.set_average(average)
            rows[average] = plan.rows(x)
            assert assert_plan_ran(plan, L, 1).startswith("stockham ")
            _check(rows[average], x, N, zoom, W, average, "short_input")
    for average in ("median", "max"):
        assert_row_close(rows[average][0], rows["mean"][0].astype(np.float64), f"short_input {average} vs mean")


def test_full_batch_no_split(oracle_lib):
    """1536 frames of the split cases' shape fill the chip without the split (31 MB of scratch,
    one chunk): picked frames against the reference, the launch not split, as mean's."""
    from pypanadapter_amd import ZoomFFT
    N, zoom, W, L, F = 1024, 1, 1024, 2560, 1536
    x = np.tile(war.burst_frames(24, L, N, zoom, W, 6000), (F // 24, 1))
    x *= (1.0 + np.arange(F, dtype=np.float32) / F)[:, None]  # every frame its own level
    with ZoomFFT(N, zoom, FS, n_win=W) as plan:
        _, split = _hooks(plan)
        plan.set_timing(True)
        plan.rows(x)
        assert_plan_ran(plan, L, F)
        assert split(plan._plan) == 1
        for average in ("median", "max"):
            plan.set_average(average)
            rows = plan.rows(x)
            assert_plan_ran(plan, L, F)
            assert split(plan._plan) == 1
            assert plan.launch_names()[-2:] == ["welch_segs", "welch_select"]
            _check(rows, x, N, zoom, W, average, "full_batch", frames=(0, 1, 767, 1535))


@pytest.mark.parametrize("N,zoom,W,L,F,welch", [(1024, 1, 1024, 2560, 12, 0), (512, 1, 300, 1536, 7, 0),
                                                (4096, 1, 512, 12288, 3, 2)])
def test_chunked_scratch_is_bit_identical(N, zoom, W, L, F, welch):
    """The frames go through the segment scratch in chunks when it would exceed the cap (here
    shrunk to 2.5 frames' worth through the test hook): the rows are those of one chunk, bit
    for bit, and every chunk reports its two intervals."""
    from pypanadapter_amd import ZoomFFT
    x = war.burst_frames(F, L, N, zoom, W, 6100 + N)
    per = war.nseg_of(L, N, zoom) * W * 4
    with ZoomFFT(N, zoom, FS, n_win=W, average="median") as plan:
        cap, _ = _hooks(plan)
        plan.set_welch(welch)
        plan.set_timing(True)
        for average in ("median", "max"):
            plan.set_average(average)
            assert cap(plan._plan, 0) == 0
            whole = plan.rows(x)
            assert " chunk=%d " % F in assert_plan_ran(plan, L, F, welch=welch)
            assert len(plan.launch_names()) == 2
            assert cap(plan._plan, per * 5 // 2) == 0
            chunked = plan.rows(x)
            assert " chunk=2 " in assert_plan_ran(plan, L, F, welch=welch, cap_bytes=per * 5 // 2)
            assert len(plan.launch_names()) == 2 * ((F + 1) // 2), plan.launch_names()
            assert whole.tobytes() == chunked.tobytes()
        assert cap(plan._plan, -1) == -1


def test_mean_after_median_is_the_fresh_plan_bytewise():
    """Mean mode keeps its kernels and rows: a plan that ran median and went back to mean gives
    a fresh plan's bytes and launches; median twice gives identical bytes."""
    from pypanadapter_amd import ZoomFFT
    N, zoom, W, L, F = 1024, 8, 128, 32768, 16
    x = war.burst_frames(F, L, N, zoom, W, 6200)
    with ZoomFFT(N, zoom, FS, n_win=W) as a, ZoomFFT(N, zoom, FS, n_win=W) as b:
        a.set_timing(True)
        b.set_timing(True)
        rows_a = a.rows(x)
        assert_plan_ran(a, L, F)
        names_a = a.launch_names()
        b.set_average("median")
        med1 = b.rows(x)
        assert_plan_ran(b, L, F)
        med2 = b.rows(x)
        assert_plan_ran(b, L, F)
        assert med1.tobytes() == med2.tobytes()
        assert not np.array_equal(med1, rows_a)
        b.set_average("mean")
        rows_b = b.rows(x)
        assert_plan_ran(b, L, F)
        assert rows_b.tobytes() == rows_a.tobytes()
        assert b.launch_names() == names_a


def test_setter_arguments():
    from pypanadapter_amd import ZoomFFT, _lib
    with ZoomFFT(64, 1, FS) as plan:
        for bad in (3, -1):
            assert plan.lib.zfft_plan_average(plan._plan, bad) == _lib.ZFFT_EINVAL
            assert b"average" in plan.lib.zfft_last_error()
        with pytest.raises(ValueError):
            plan.set_average("mode")
        assert plan.average == "mean"
        plan.set_average("max")
        assert plan.average == "max"


def test_psd_row_average_and_the_cached_mean_plan():
    """psd_row(average=...) is the plan's rows, and a detector call between two mean calls
    leaves the cached mean plan (and its rows) alone."""
    from pypanadapter_amd import ZoomFFT, panadapter
    N, zoom, W, L = 1024, 1, 1024, 9216
    x = war.burst_frame(L, N, zoom, W, 6300)
    mean1 = panadapter.psd_row(x, FS, N, zoom)
    mean_plan = panadapter._cache(0).plan
    med = panadapter.psd_row(x, FS, N, zoom, average="median")
    with ZoomFFT(N, zoom, FS, n_win=W, average="median") as plan:
        assert plan.average == "median"
        plan.set_timing(True)
        np.testing.assert_array_equal(med, plan.rows(x).astype(np.float64))
        assert_plan_ran(plan, L, 1)
    mean2 = panadapter.psd_row(x, FS, N, zoom)
    assert panadapter._cache(0).plan is mean_plan
    np.testing.assert_array_equal(mean1, mean2)
    assert not np.array_equal(mean1, med)
    thr = panadapter.thread_psd_row(x, FS, N, zoom, average="max")
    np.testing.assert_array_equal(thr, panadapter.psd_row(x, FS, N, zoom, average="max"))
    assert not np.array_equal(thr, med)


def test_ring_process_inherits_the_plan_mode():
    from pypanadapter_amd import IQRing, ZoomFFT
    N, W, L = 1024, 1024, 9216
    x = war.burst_frame(L, N, 1, W, 6400)
    ring = IQRing(chunk_size=L)
    with ZoomFFT(N, 1, FS, n_win=W, average="max") as plan:
        plan.set_timing(True)
        want = plan.rows(x)
        assert_plan_ran(plan, L, 1)
        ring.add(x)
        got = ring.process(plan)
    ring.close()
    np.testing.assert_array_equal(got, want)
