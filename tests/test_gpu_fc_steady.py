"""The FC decimator's steady state at the smallest shape that has one (fc_kernels.hip, DESIGN
§3.9): 1024 frames per call, so one workgroup walks a whole frame of five blocks -- block 0 loads
its window sample by sample (the edge path), blocks 1.. take theirs from the registers carried
over and the prefetch, the last block is on the edge path again -- and both transitions between
the two paths happen.  Rows of three picked frames (the others are zero) against the float64
oracle; the few-frame tests of test_gpu_fc.py never carry, and its batch tests run 45 blocks."""
import numpy as np
import pytest

from conftest import assert_row_close
from test_gpu_pc import _encode, _frames

pytestmark = pytest.mark.gpu

F_ALL, N = 1024, 1024
PICKS = (0, 511, F_ALL - 1)
L8 = 29701               # zoom 8: L mod 8 = 5, ceil(L / 8) = 3713 outputs = 4 blocks of 832 + 385
L4 = 4 * 7168 + 3        # zoom 4: 7169 outputs = 4 blocks of 1792 + 1


@pytest.fixture(scope="module", autouse=True)
def _gpu(zfft_lib):
    from pypanadapter_amd import device_count
    assert device_count() >= 1, "GPU tests need a HIP device"


def _paths(L, zoom, bpc=None):
    """'edge' / 'carried' per block of a frame, from the kernel's geometry (Geo<Z>: a block
    advances 512 S samples from K before its first output; a window is 8192 samples).  A block is
    carried when it is not the first of its run and its window lies inside the frame."""
    S, K = (13, 768) if zoom == 8 else (14, 512)
    P = 512 * S // zoom
    nd = -(-L // zoom)
    nb = -(-nd // P)
    bpc = bpc or nb
    inside = [512 * S * b - K >= 0 and 512 * S * b - K + 8192 <= L for b in range(nb)]
    return ["carried" if inside[b] and b % bpc else "edge" for b in range(nb)]


def test_shapes_walk_both_paths():
    assert _paths(L8, 8) == ["edge", "carried", "carried", "carried", "edge"]
    p4 = _paths(L4, 4)
    assert p4[0] == "edge" and p4[-1] == "edge" and p4.count("carried") >= 2, p4
    # 512 frames per call: two runs per frame, block 3 first of the second one
    assert _paths(L8, 8, bpc=3) == ["edge", "carried", "carried", "edge", "edge"]


_CACHE = {}


def _input(zoom, L):
    """(device tensor of F_ALL complex64 frames, {picked frame: its samples}), made once."""
    import torch
    key = (zoom, L)
    if key not in _CACHE:
        W = N // zoom
        dev = torch.device("cuda:0")
        x = torch.zeros((F_ALL, L, 2), device=dev, dtype=torch.float32)
        xs = {f: _frames(1, L, N, zoom, W, seed0=8700 + 10 * zoom + f)[0] for f in PICKS}
        for f, v in xs.items():
            x[f] = torch.from_numpy(np.ascontiguousarray(v).view(np.float32).reshape(L, 2)).to(dev)
        _CACHE.clear()          # one 243 MB batch on the device at a time
        _CACHE[key] = (x, xs)
    return _CACHE[key]


def _run(zoom, x, L, F, in_dtype=None):
    import torch
    from pypanadapter_amd import ZoomFFT
    W = N // zoom
    rows = torch.empty((F, W), device=x.device, dtype=torch.float32)
    kw = {} if in_dtype is None else {"in_dtype": in_dtype}
    with ZoomFFT(N, zoom, 2.4e6, n_win=W, **kw) as plan:
        plan.set_path(6)
        plan.set_timing(True)
        plan.process_device(x.data_ptr(), L, F, rows.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        names = plan.launch_names()
    assert "fc_decim" in names, names
    return rows.cpu().numpy(), names


@pytest.mark.parametrize("zoom,L", [(4, L4), (8, L8)], ids=["zoom4", "zoom8"])
def test_fc_steady_rows_vs_oracle(oracle_lib, zoom, L):
    x, xs = _input(zoom, L)
    got, _ = _run(zoom, x, L, F_ALL)
    for f in PICKS:
        assert_row_close(got[f], oracle_lib.psd_row(xs[f], 2.4e6, N, zoom, N // zoom), f"zoom {zoom} frame {f}")


def test_fc_steady_complex32_vs_oracle(oracle_lib):
    """complex32 holds 14 of its 16 filter-table pairs in registers (complex64: 8), so its
    block loop waits on other loads."""
    import torch
    _, xs = _input(8, L8)
    dev = torch.device("cuda:0")
    x = torch.zeros((F_ALL, L8, 2), device=dev, dtype=torch.float16)
    vals = {}
    for f, v in xs.items():
        h, vals[f] = _encode(v, "complex32")
        x[f] = torch.from_numpy(h.reshape(L8, 2)).to(dev)
    got, _ = _run(8, x, L8, F_ALL, in_dtype="complex32")
    for f in PICKS:
        assert_row_close(got[f], oracle_lib.psd_row(vals[f], 2.4e6, N, 8, N // 8), f"complex32 frame {f}")


def test_fc_steady_block_on_either_path_same_rows():
    """The first 512 frames alone: each frame then splits into two runs of blocks, and block 3,
    carried in the 1024-frame call, is the first of a run and loads its window on the edge path.
    Both paths hand the same fp32 values to the same arithmetic, so the decimated IQ is the same;
    the rows are bit-equal when the Welch stage that follows runs the same kernels in both calls,
    and within the row tolerance of the suite when the schedule picks another Welch form for the
    smaller batch."""
    x, _ = _input(8, L8)
    full, names_full = _run(8, x, L8, F_ALL)
    half, names_half = _run(8, x, L8, F_ALL // 2)
    print("kernels at 1024 frames:", names_full, "at 512:", names_half)
    if list(names_full) == list(names_half):
        np.testing.assert_array_equal(half, full[:F_ALL // 2])
    else:
        for f in (p for p in PICKS if p < F_ALL // 2):
            assert_row_close(half[f], full[f], f"frame {f}")
