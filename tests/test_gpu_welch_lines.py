"""GPU checks of the time-resolved waterfall (zfft_plan_segments_per_line: R = ceil(nseg / g)
rows per frame, each the plan's detector over g consecutive Welch segments) against the float64
reference of welch_lines_ref.py (pinned on the CPU by test_welch_lines.py), per line under the
project's row gate (conftest.assert_row_close: 1e-3 dB within 100 dB of the line's peak, 1e-5 of
the peak amplitude).  The inputs carry a burst in one or two segments, so the lines differ by
tens of dB at its bins and a wrong group boundary or line order fails.  The shapes are the
smallest that reach each Welch kernel family and form; every case runs the three detectors.

Worst errors these tests printed on an MI355X: profiles/wlines/test_errors.json."""
import ctypes

import numpy as np
import pytest

import welch_average_ref as war
import welch_lines_ref as wlr
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


def _route(plan, route):
    """Mean lines: 0 the plan's own route (fused where a fused kernel exists), 1 the segment
    scratch everywhere."""
    hook = plan.lib.zfft__plan_lines_route
    hook.argtypes, hook.restype = [ctypes.c_void_p, ctypes.c_int], ctypes.c_int
    assert hook(plan._plan, route) == 0


def _check(lines, x, N, zoom, W, g, average, what, frames=None):
    """lines (F, R, row length) against the reference, line by line; the worst errors printed."""
    worst = (0.0, 0.0)
    for f in (range(len(x)) if frames is None else frames):
        ref = wlr.ref_lines(x[f], FS, N, zoom, W, g, average)
        assert lines[f].shape == ref.shape, (what, lines[f].shape, ref.shape)
        for r in range(len(ref)):
            worst = tuple(max(a, b) for a, b in zip(worst, row_errors(lines[f][r], ref[r])))
            assert_row_close(lines[f][r], ref[r], f"{what} g={g} {average} frame {f} line {r}")
    print(f"{what} g={g} {average}: max|ddB|={worst[0]:.3e} max|damp|={worst[1]:.3e}")


def _recombined(lines, nseg, g):
    """The frame's mean row from its mean lines: 20 log10(sum_r n_r 10^(line_r / 20) / nseg)."""
    R = lines.shape[-2]
    n = np.array([min(g, nseg - r * g) for r in range(R)], dtype=np.float64)
    amp = 10.0 ** (lines.astype(np.float64) / 20.0)
    return 20.0 * np.log10((amp * n[:, None]).sum(axis=-2) / nseg)


_SEL_L = 64 + 32 * 599

# name: (N, zoom, W, L, frames, gs, options)
CASES = {
    # Stockham kernel (N < 1024): 11 segments in groups of 4, 4, 3; behind zoom 2 at g = 1
    "stockham_n64_groups_4_4_3": (64, 1, 64, 64 + 32 * 10, 2, (4,), {}),
    "stockham_n512_zoom2": (512, 2, 256, 8192, 2, (1,), {}),
    # in-place DIF, several frames per workgroup (5 frames: a spare frame slot), 17 segments:
    # tails 0, 2, 1; group sizes even and odd for the median
    "dif1024_nseg17": (1024, 1, 1024, 9216, 5, (1, 5, 16), {}),
    # DIF N = 4096 pruned behind the automatic decimator, and FC in front of N = 1024
    "dif4096_pruned_zoom8": (4096, 8, 512, 98304, 1, (2,), {}),
    "dif1024_fc_in_front": (1024, 8, 128, 32768, 16, (3,), {"first": "fc_decim"}),
    "dif4096_full": (4096, 1, 4096, 20480, 1, (4,), {}),
    "dif16384_pruned": (16384, 1, 2048, 65536, 1, (3,), {}),
    "dif16384_full": (16384, 1, 16384, 65536, 1, (3,), {}),
    # the split few-frames form
    "split_1_frame": (1024, 1, 1024, 9216, 1, (1, 4, 16), {"split": True}),
    "split_2_frames": (1024, 1, 1024, 9216, 2, (1, 4, 16), {"split": True}),
    # four-step, pruned and full, and forced at N = 4096
    "four_32768_pruned": (32768, 1, 4096, 163840, 2, (4,), {}),
    "four_32768_full": (32768, 1, 32768, 163840, 2, (4,), {}),
    "four_65536": (65536, 1, 8192, 327680, 2, (4,), {}),
    "four_4096_forced": (4096, 1, 512, 20480, 2, (4,), {"welch": 2}),
    # one-sided rows: real input at zoom 1, even and odd W
    "onesided_even_w": (1024, 1, 1024, 9216, 2, (5,), {"real": True}),
    "onesided_odd_w": (1024, 1, 301, 9216, 2, (5,), {"real": True}),
    # welch_select's thresholds on the group size: registers <= 32 < LDS <= 256 < scratch
    "select_thresholds": (64, 1, 50, _SEL_L, 2, (32, 33, 256, 257), {}),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_lines_vs_float64_reference(oracle_lib, name):
    """Every line within the gate of the reference; max decomposes (the largest of a frame's
    max lines is its g = 0 max row, bytewise: the same segment pass, log10f of the same value);
    mean recombines (the lines' weighted mean is the g = 0 mean row within the gate)."""
    from pypanadapter_amd import ZoomFFT
    N, zoom, W, L, F, gs, opt = CASES[name]
    real = opt.get("real", False)
    nseg = war.nseg_of(L, N, zoom)
    x = war.burst_frames(F, L, N, zoom, W, 7000 + 13 * sorted(CASES).index(name), real=real)
    with ZoomFFT(N, zoom, FS, n_win=W, in_dtype="f32" if real else "complex64") as plan:
        _, split = _hooks(plan)
        plan.set_timing(True)
        if "welch" in opt:
            plan.set_welch(opt["welch"])
        for average in MODES:
            plan.set_average(average)
            plan.set_segments_per_line(0)
            whole = plan.rows(x)
            welch = opt.get("welch", 0)
            assert_plan_ran(plan, L, F, welch=welch)
            assert whole.shape == (F, plan.row_length)
            if opt.get("split") and average == "mean":  # the shape is in the split regime
                assert split(plan._plan) > 1
            for g in gs:
                plan.set_segments_per_line(g)
                R = wlr.line_count(nseg, g)
                assert plan.lines(L) == R and R > 1
                lines = plan.rows(x)
                desc = assert_plan_ran(plan, L, F, welch=welch)
                assert (" lines " in desc) == (average == "mean" and 1024 <= N <= 16384 and welch != 2), desc
                assert lines.shape == (F, R, plan.row_length)
                if "first" in opt:
                    assert plan.launch_names()[0] == opt["first"], plan.launch_names()
                _check(lines, x, N, zoom, W, g, average, name)
                if average == "max":
                    assert lines.max(axis=1).tobytes() == whole.tobytes(), (name, g)
                if average == "mean":  # the other route for mean lines, against the same reference
                    _route(plan, 1)
                    _check(plan.rows(x), x, N, zoom, W, g, average, name + "/scratch")
                    assert "select=mean_lines" in assert_plan_ran(plan, L, F, welch=welch, lines_route=1)
                    _route(plan, 0)
                    for f in range(F):
                        assert_row_close(_recombined(lines[f], nseg, g), whole[f].astype(np.float64),
                                         f"{name} g={g} frame {f} recombined")


@pytest.mark.parametrize("g", [2, 3])
def test_full_batch(oracle_lib, g):
    """1536 frames of 4 segments fill the chip without the split: 24 distinct frames tiled 64
    times, every tile bytewise its first occurrence and the first occurrences against the
    reference, so no frame is left unchecked."""
    from pypanadapter_amd import ZoomFFT
    N, zoom, W, L, F = 1024, 1, 1024, 2560, 1536
    x24 = war.burst_frames(24, L, N, zoom, W, 7500)
    x = np.tile(x24, (F // 24, 1))
    assert war.nseg_of(L, N, zoom) == 4
    with ZoomFFT(N, zoom, FS, n_win=W, segments_per_line=g) as plan:
        _, split = _hooks(plan)
        plan.set_timing(True)
        for average in MODES:
            plan.set_average(average)
            lines = plan.rows(x)
            assert_plan_ran(plan, L, F)
            assert split(plan._plan) == 1
            assert lines.shape == (F, 2, W)
            tiles = lines.reshape(F // 24, 24, 2, W)
            for t in range(1, F // 24):
                assert tiles[t].tobytes() == tiles[0].tobytes(), (average, t)
            _check(lines, x24, N, zoom, W, g, average, "full_batch", frames=range(24))


def test_g0_is_unchanged_bytewise():
    """A plan set to 3 segments per line and back to 0 gives a fresh plan's bytes and launches,
    in all three detectors; g >= nseg gives those bytes too, as (F, 1, W)."""
    from pypanadapter_amd import ZoomFFT
    N, zoom, W, L, F = 1024, 8, 128, 32768, 16
    nseg = war.nseg_of(L, N, zoom)
    x = war.burst_frames(F, L, N, zoom, W, 7600)
    with ZoomFFT(N, zoom, FS, n_win=W) as a, ZoomFFT(N, zoom, FS, n_win=W) as b:
        a.set_timing(True)
        b.set_timing(True)
        for average in MODES:
            a.set_average(average)
            b.set_average(average)
            fresh = a.rows(x)
            assert_plan_ran(a, L, F)
            names = a.launch_names()
            b.set_segments_per_line(3)
            lines = b.rows(x)
            assert_plan_ran(b, L, F)
            assert lines.shape == (F, wlr.line_count(nseg, 3), W)
            b.set_segments_per_line(0)
            back = b.rows(x)
            assert_plan_ran(b, L, F)
            assert back.shape == fresh.shape and back.tobytes() == fresh.tobytes(), average
            assert b.launch_names() == names
            for g in (nseg, nseg + 1, 1000):
                b.set_segments_per_line(g)
                one = b.rows(x)
                assert_plan_ran(b, L, F)
                assert one.shape == (F, 1, W)
                assert one.tobytes() == fresh.tobytes(), (average, g)
                assert b.launch_names() == names
            b.set_segments_per_line(0)


def test_short_input_branch():
    """L_d = 624 < N: one segment, so any g gives one line, (1, W) for a single frame, with the
    bytes of g = 0."""
    from pypanadapter_amd import ZoomFFT
    N, zoom, W, L = 2048, 512, 2048, 319488
    x = war.burst_frames(1, L, N, zoom, W, 7700)[0]
    with ZoomFFT(N, zoom, FS, n_win=W) as plan:
        plan.set_timing(True)
        for average in MODES:
            plan.set_average(average)
            plan.set_segments_per_line(0)
            row = plan.rows(x)
            assert_plan_ran(plan, L, 1)
            assert row.shape == (W,)
            for g in (1, 2, 7):
                plan.set_segments_per_line(g)
                assert plan.lines(L) == 1
                lines = plan.rows(x)
                assert " lines=1 " in assert_plan_ran(plan, L, 1)
                assert lines.shape == (1, W)
                assert lines.tobytes() == row.tobytes(), (average, g)


@pytest.mark.parametrize("N,zoom,W,L,F,g,welch", [(1024, 1, 1024, 2560, 12, 2, 0), (4096, 1, 512, 12288, 3, 2, 2)])
def test_chunked_scratch_is_bit_identical(N, zoom, W, L, F, g, welch):
    """The segment scratch holds segments, not lines: with its cap shrunk to 2.5 frames' worth
    the frames go in chunks and the lines are those of one chunk, bit for bit; the same call
    twice gives identical bytes."""
    from pypanadapter_amd import ZoomFFT
    x = war.burst_frames(F, L, N, zoom, W, 7800 + N)
    per = war.nseg_of(L, N, zoom) * W * 4
    with ZoomFFT(N, zoom, FS, n_win=W, segments_per_line=g) as plan:
        cap, _ = _hooks(plan)
        _route(plan, 1)  # mean lines through the scratch as well (their fused form has none)
        plan.set_welch(welch)
        plan.set_timing(True)
        for average in MODES:
            plan.set_average(average)
            assert cap(plan._plan, 0) == 0
            whole = plan.rows(x)
            assert " chunk=%d " % F in assert_plan_ran(plan, L, F, welch=welch, lines_route=1)
            assert len(plan.launch_names()) == 2
            assert plan.rows(x).tobytes() == whole.tobytes()
            assert cap(plan._plan, per * 5 // 2) == 0
            chunked = plan.rows(x)
            assert " chunk=2 " in assert_plan_ran(plan, L, F, welch=welch, lines_route=1, cap_bytes=per * 5 // 2)
            assert len(plan.launch_names()) == 2 * ((F + 1) // 2), plan.launch_names()
            assert whole.tobytes() == chunked.tobytes(), average


def test_host_batching_offsets_rows_by_lines(oracle_lib):
    """A host call above the 64 MB pipelining threshold runs in two batches; its bytes are those
    of the same frames in two separate calls -- a per-batch row offset without the factor R
    would overwrite the first batch's lines."""
    from pypanadapter_amd import ZoomFFT
    N, zoom, W, L, F, g = 1024, 8, 128, 32768, 272, 3
    x16 = war.burst_frames(16, L, N, zoom, W, 7900)
    x = np.tile(x16, (F // 16, 1))
    assert x.nbytes >= 64 << 20 and x[:F // 2].nbytes < 64 << 20
    with ZoomFFT(N, zoom, FS, n_win=W, segments_per_line=g) as plan:
        plan.set_timing(True)
        for average in MODES:
            plan.set_average(average)
            both = plan.rows(x)
            assert_plan_ran(plan, L, F // 2)  # (the last of two batches)
            assert "batch_wait" in plan.launch_names()
            halves = np.concatenate([plan.rows(x[:F // 2]), plan.rows(x[F // 2:])])
            assert "batch_wait" not in plan.launch_names()
            assert both.shape == halves.shape == (F, 3, W)
            assert both.tobytes() == halves.tobytes(), average
            _check(both, x, N, zoom, W, g, average, "host_batching", frames=(0, F // 2, F - 1))


def test_setter_arguments_and_shapes():
    from pypanadapter_amd import ZoomFFT, _lib
    N, W, L = 64, 64, 64 + 32 * 10
    x = war.burst_frames(3, L, N, 1, W, 8000)
    with ZoomFFT(N, 1, FS, n_win=W) as plan:
        assert plan.segments_per_line == 0
        assert plan.lib.zfft_plan_segments_per_line(plan._plan, -1) == _lib.ZFFT_EINVAL
        assert b"segments_per_line" in plan.lib.zfft_last_error()
        with pytest.raises(ValueError):
            plan.set_segments_per_line(-2)
        assert plan.segments_per_line == 0
        assert plan.rows(x).shape == (3, W) and plan.rows(x[0]).shape == (W,)
        assert plan.lines(L) == 1 and plan.line_times(L).shape == (1,)
        plan.set_segments_per_line(4)
        assert plan.segments_per_line == 4 and plan.lines(L) == 3
        assert plan.rows(x).shape == (3, 3, W) and plan.rows(x[0]).shape == (3, W)
        np.testing.assert_array_equal(plan.rows(x)[1], plan.rows(x[1]))
        t = plan.line_times(L)
        assert t.shape == (3,) and np.all(np.diff(t) > 0) and 0 < t[0] and t[-1] < L / FS
        np.testing.assert_allclose(t, wlr.ref_line_times(L, FS, N, 1, 4), rtol=1e-12)
    with ZoomFFT(N, 1, FS, n_win=W, segments_per_line=4, average="max") as plan:
        assert plan.segments_per_line == 4 and plan.rows(x).shape == (3, 3, W)


def test_psd_lines_and_the_cached_row_plan():
    """psd_lines is the plan's lines widened to float64, and a psd_lines call between two
    psd_row calls leaves the cached psd_row plan alone."""
    from pypanadapter_amd import ZoomFFT, panadapter
    N, zoom, W, L, g = 1024, 1, 1024, 9216, 5
    x = war.burst_frame(L, N, zoom, W, 8100)
    row1 = panadapter.psd_row(x, FS, N, zoom)
    row_plan = panadapter._cache(0).plan
    for average in MODES:
        lines = panadapter.psd_lines(x, FS, N, zoom, g, average=average)
        assert lines.shape == (4, W) and lines.dtype == np.float64
        with ZoomFFT(N, zoom, FS, n_win=W, segments_per_line=g, average=average) as plan:
            np.testing.assert_array_equal(lines, plan.rows(x).astype(np.float64))
    row2 = panadapter.psd_row(x, FS, N, zoom)
    assert panadapter._cache(0).plan is row_plan
    np.testing.assert_array_equal(row1, row2)
    whole = panadapter.psd_lines(x, FS, N, zoom, 0)
    assert whole.shape == (1, W)
    np.testing.assert_array_equal(whole[0], row1)


def test_ring_process_gives_the_frames_lines():
    from pypanadapter_amd import IQRing, ZoomFFT, _lib
    N, W, L, g = 1024, 1024, 9216, 5
    x = war.burst_frame(L, N, 1, W, 8200)
    ring = IQRing(chunk_size=L)
    with ZoomFFT(N, 1, FS, n_win=W, average="median", segments_per_line=g) as plan:
        want = plan.rows(x)
        assert want.shape == (4, W)
        ring.add(x)
        got = ring.process(plan)
        assert got.shape == (4, W)
        np.testing.assert_array_equal(got, want)
        ring.add(x[:N - 1])  # shorter than fft_size: skipped, the frame still drained
        assert ring.process(plan) is None
        assert ring.state() == (0, 0, 0)
        # the one-row entry point refuses a lines plan before it takes the frame
        ring.add(x)
        before = ring.state()
        row = np.empty(W, np.float32)
        produced = ctypes.c_int32(5)
        rc = ring.lib.zfft_ring_process(ring._ring, plan._plan, row.ctypes.data_as(ctypes.c_void_p),
                                        ctypes.byref(produced))
        assert rc == _lib.ZFFT_EINVAL and produced.value == 0
        assert b"zfft_ring_process_lines" in ring.lib.zfft_last_error()
        assert ring.state() == before
        # a buffer one line short of what the ring's capacity can give: refused, nothing taken
        cap = plan.lines(ring.max_size)
        assert cap == ring.lib.zfft_line_count(ring.max_size, 1, N, g) > 4
        rows = np.empty((cap, W), np.float32)
        rc = ring.lib.zfft_ring_process_lines(ring._ring, plan._plan, rows.ctypes.data_as(ctypes.c_void_p),
                                              cap - 1, ctypes.byref(produced))
        assert rc == _lib.ZFFT_EINVAL and produced.value == 0
        assert ring.state() == before
        rc = ring.lib.zfft_ring_process_lines(ring._ring, plan._plan, rows.ctypes.data_as(ctypes.c_void_p),
                                              cap, ctypes.byref(produced))
        assert rc == 0 and produced.value == 4
        np.testing.assert_array_equal(rows[:4], want)
        assert ring.state() == (0, 0, 0)
    ring.close()


def test_waterfall_takes_the_lines_of_a_device_call():
    """The F R device rows of a lines plan pushed in one waterfall_push_device(count = F R) give
    the image of the same rows pushed one by one from the host; push(None) is the newest line."""
    import torch
    from pypanadapter_amd import ZoomFFT
    N, W, L, F, g = 1024, 1024, 9216, 2, 5
    x = war.burst_frames(F, L, N, 1, W, 8300)
    dev = torch.device("cuda:0")
    xd = torch.from_numpy(np.ascontiguousarray(x).view(np.float32).reshape(F, L, 2)).to(dev)
    with ZoomFFT(N, 1, FS, n_win=W, segments_per_line=g) as a, ZoomFFT(N, 1, FS, n_win=W) as b:
        R = a.lines(L)
        rows = torch.empty((F * R, W), device=dev, dtype=torch.float32)
        st = torch.cuda.current_stream().cuda_stream
        a.process_device(xd.data_ptr(), L, F, rows.data_ptr(), st)
        a.waterfall_push_device(rows.data_ptr(), F * R, st)
        a.waterfall_push(None)
        torch.cuda.synchronize()
        host = rows.cpu().numpy()
        np.testing.assert_array_equal(host.reshape(F, R, W), a.rows(x))
        for r in host:
            b.waterfall_push(r)
        b.waterfall_push(host[-1])
        np.testing.assert_array_equal(a.waterfall_image(), b.waterfall_image())
