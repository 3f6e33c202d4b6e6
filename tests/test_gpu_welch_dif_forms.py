"""GPU checks of the in-place DIF Welch kernel (welch_dif_kernel) in the forms the
batch path runs and the few-frame tests do not: one workgroup per frame over all of the frame's
segments (no split), where the window stays in registers across the segments, the next segment's
values are requested at the segment head into one of two arrays used in turn, and the segment
mean is summed between lanes.  Rows against the float64 oracle (oracle.coracle.psd_row) under
the suite's row gate (conftest.assert_row_close: 1e-3 dB within 100 dB of the peak,
1e-5 of the peak amplitude -- bench.py's parity_check).

Segment counts: 1 (no prefetch consumer), 2 and 3 (both prefetch arrays, odd and even tails), 4
and 5 in the smallest batch that runs unsplit (384 frames at N = 4096: welch_split gives 1 from
half the chip's workgroups on).  N = 1024 and 2048 put several frames in a workgroup, with a
spare frame slot at 5 frames; N = 16384 is the 1024-thread frame that holds no window."""
import ctypes

import numpy as np
import pytest

import welch_average_ref as war
import welch_lines_ref as wlr
from conftest import assert_row_close, row_errors

pytestmark = pytest.mark.gpu
FS = war.FS


def _split(plan):
    hook = plan.lib.zfft__plan_welch_split
    hook.argtypes, hook.restype = [ctypes.c_void_p], ctypes.c_int
    return hook(plan._plan)


def _frames(F, L, N, zoom, W, seed0):
    from pypanadapter_amd import synth
    return np.stack([synth.make_iq(L, FS, seed0 + f, n_fft=N, zoom=zoom, n_win=W) for f in range(F)])


def _check_rows(oracle_lib, rows, x, N, zoom, W, what, frames=None):
    worst = (0.0, 0.0)
    for f in (range(len(x)) if frames is None else frames):
        ref = oracle_lib.psd_row(x[f], FS, N, zoom, W)
        worst = tuple(max(a, b) for a, b in zip(worst, row_errors(rows[f], ref)))
        assert_row_close(rows[f], ref, f"{what} frame {f}")
    print(f"{what}: max|ddB|={worst[0]:.3e} max|damp|={worst[1]:.3e}")


@pytest.mark.parametrize("nseg", [1, 2, 3])
def test_few_frames_unsplit(oracle_lib, nseg):
    """N = 4096 behind zoom 8, 2 frames of 1, 2 and 3 segments: below 4 segments a frame is not
    split, so one workgroup walks all of them."""
    from pypanadapter_amd import ZoomFFT
    N, zoom, W, F = 4096, 8, 512, 2
    L = zoom * (N + (nseg - 1) * N // 2)
    assert war.nseg_of(L, N, zoom) == nseg
    x = _frames(F, L, N, zoom, W, 9100 + nseg)
    with ZoomFFT(N, zoom, FS, n_win=W) as plan:
        plan.set_timing(True)
        rows = plan.rows(x)
        assert plan.launch_names()[-1] == "welch_rows", plan.launch_names()
        assert _split(plan) == 1
        _check_rows(oracle_lib, rows, x, N, zoom, W, f"few_frames nseg={nseg}")
        assert plan.rows(x).tobytes() == rows.tobytes()


@pytest.mark.parametrize("nseg", [4, 5])
def test_batch_unsplit(oracle_lib, nseg):
    """384 frames of N = 4096 behind zoom 8, the smallest batch that runs one workgroup per frame:
    five distinct frames spread over the batch, frames 0, 191 and 383 against the oracle; then
    every frame a copy of frame 0, and all 384 rows bit-equal."""
    import torch
    from pypanadapter_amd import ZoomFFT
    N, zoom, W, F = 4096, 8, 512, 384
    L = zoom * (N + (nseg - 1) * N // 2)
    assert war.nseg_of(L, N, zoom) == nseg
    x5 = _frames(5, L, N, zoom, W, 9200 + nseg)
    idx = np.arange(F) % 5
    assert len({int(idx[f]) for f in (0, 191, 383)}) == 3
    dev = torch.device("cuda:0")
    xd5 = torch.from_numpy(np.ascontiguousarray(x5).view(np.float32).reshape(5, L, 2)).to(dev)
    rows = torch.empty((F, W), device=dev, dtype=torch.float32)
    st = torch.cuda.current_stream().cuda_stream
    with ZoomFFT(N, zoom, FS, n_win=W) as plan:
        plan.set_timing(True)
        xd = xd5[torch.from_numpy(idx).to(dev)].contiguous()
        plan.process_device(xd.data_ptr(), L, F, rows.data_ptr(), st)
        torch.cuda.synchronize()
        assert plan.launch_names()[-1] == "welch_rows", plan.launch_names()
        assert _split(plan) == 1
        host = rows.cpu().numpy()
        for f in (0, 191, 383):
            ref = oracle_lib.psd_row(x5[idx[f]], FS, N, zoom, W)
            ddb, damp = row_errors(host[f], ref)
            print(f"batch nseg={nseg} frame {f}: max|ddB|={ddb:.3e} max|damp|={damp:.3e}")
            assert_row_close(host[f], ref, f"batch nseg={nseg} frame {f}")
        xd = xd5[torch.zeros(F, dtype=torch.int64, device=dev)].contiguous()
        plan.process_device(xd.data_ptr(), L, F, rows.data_ptr(), st)
        torch.cuda.synchronize()
        same = rows.cpu().numpy()
        assert same[0].tobytes() == host[0].tobytes()
        assert all(same[f].tobytes() == same[0].tobytes() for f in range(1, F))


@pytest.mark.parametrize("N,zoom", [(1024, 4), (1024, 8), (2048, 4), (2048, 8)])
def test_shared_workgroup(oracle_lib, N, zoom):
    """N = 1024 (4 frames per workgroup) and 2048 (2), 5 frames of 3 segments: a spare frame slot
    in the last workgroup."""
    from pypanadapter_amd import ZoomFFT
    W, F = N // zoom, 5
    L = zoom * 2 * N
    assert war.nseg_of(L, N, zoom) == 3
    x = _frames(F, L, N, zoom, W, 9300 + N + zoom)
    with ZoomFFT(N, zoom, FS, n_win=W) as plan:
        plan.set_timing(True)
        rows = plan.rows(x)
        assert plan.launch_names()[-1] == "welch_rows", plan.launch_names()
        assert _split(plan) == 1
        _check_rows(oracle_lib, rows, x, N, zoom, W, f"shared N={N} zoom={zoom}")


@pytest.mark.parametrize("nseg", [2, 3])
def test_large_frame(oracle_lib, nseg):
    """N = 16384 behind zoom 8: one 1024-thread workgroup per frame, stage-1 stores past the
    offset field's reach through the second base."""
    from pypanadapter_amd import ZoomFFT
    N, zoom, W, F = 16384, 8, 2048, 2
    L = zoom * (N + (nseg - 1) * N // 2)
    assert war.nseg_of(L, N, zoom) == nseg
    x = _frames(F, L, N, zoom, W, 9400 + nseg)
    with ZoomFFT(N, zoom, FS, n_win=W) as plan:
        plan.set_timing(True)
        rows = plan.rows(x)
        assert plan.launch_names()[-1] == "welch_rows", plan.launch_names()
        assert _split(plan) == 1
        _check_rows(oracle_lib, rows, x, N, zoom, W, f"large nseg={nseg}")


def test_segment_and_line_forms(oracle_lib):
    """SEG (the median detector) and LINES (segments_per_line = 2) at N = 4096 behind zoom 8, 2
    frames of 5 segments, against the references of test_gpu_welch_average.py and
    test_gpu_welch_lines.py."""
    from pypanadapter_amd import ZoomFFT
    N, zoom, W, F, g = 4096, 8, 512, 2, 2
    L = zoom * (N + 4 * N // 2)
    assert war.nseg_of(L, N, zoom) == 5
    x = war.burst_frames(F, L, N, zoom, W, 9500)
    with ZoomFFT(N, zoom, FS, n_win=W, average="median") as plan:
        plan.set_timing(True)
        rows = plan.rows(x)
        assert plan.launch_names()[-2:] == ["welch_segs", "welch_select"], plan.launch_names()
        for f in range(F):
            assert_row_close(rows[f], war.ref_row(x[f], FS, N, zoom, W, "median"), f"median frame {f}")
    with ZoomFFT(N, zoom, FS, n_win=W, segments_per_line=g) as plan:
        plan.set_timing(True)
        lines = plan.rows(x)
        assert plan.launch_names()[-1] == "welch_lines", plan.launch_names()
        assert lines.shape == (F, 3, W)
        for f in range(F):
            ref = wlr.ref_lines(x[f], FS, N, zoom, W, g, "mean")
            for r in range(3):
                assert_row_close(lines[f][r], ref[r], f"lines frame {f} line {r}")
