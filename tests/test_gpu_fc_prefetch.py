"""The FC decimator's spread prefetch, table hold and buffer stores (fc_kernels.hip,
fc_prefetch_plan.h) at the steady-state shape of test_gpu_fc_steady.py -- 1024 frames
per call, five blocks per frame: edge, carried, carried, carried, edge -- for the instantiations
that file leaves out: cu8, real f32, complex32 at zoom 4 and np.flip for complex64.  Each is a
kernel of its own, with its own group plan and hold.

Three frames are non-zero, two of them adjacent: the outputs are stored by every lane through a
buffer resource that ends with the block's last output of the frame, and a store the range check
should drop and did not would land in the first outputs of the next frame.  Rows against the
float64 oracle, with the suite's row tolerance.

The decimated IQ itself is only returned for one frame per call (zfft_decimate; every block is
then the first of a run): the picked frames' IQ against the oracle under test_gpu_fc.py's FC_TOL
covers the stores and the frame's last, partly filled block for every format; the carried blocks
are covered by the rows."""
import numpy as np
import pytest

from conftest import assert_row_close, check_rel
from test_gpu_fc import FC_TOL
from test_gpu_fc_steady import L4, L8, _paths
from test_gpu_pc import _encode, _frames

pytestmark = pytest.mark.gpu

F_ALL, N = 1024, 1024
PICKS = (0, 510, 511)        # 510 and 511 adjacent; all three inside the 512-frame call as well
TORCH_DT = {"complex64": "float32", "complex32": "float16", "cu8": "uint8", "f32": "float32"}
# zoom, L, input format, flip
CASES = [(8, L8, "cu8", False), (8, L8, "cu8", True), (4, L4, "cu8", False),
         (8, L8, "f32", False), (4, L4, "f32", True),
         (4, L4, "complex32", False),
         (8, L8, "complex64", True), (4, L4, "complex64", True)]


@pytest.fixture(scope="module", autouse=True)
def _gpu(zfft_lib):
    from pypanadapter_amd import device_count
    assert device_count() >= 1, "GPU tests need a HIP device"


_SRC = {}


def _source(zoom, L):
    """{picked frame: complex64 samples}, made once per (zoom, L)."""
    if (zoom, L) not in _SRC:
        _SRC[(zoom, L)] = {f: _frames(1, L, N, zoom, N // zoom, seed0=9100 + 10 * zoom + f)[0] for f in PICKS}
    return _SRC[(zoom, L)]


def _batch(zoom, L, fmt):
    """(device tensor of F_ALL frames in `fmt`, {frame: raw array}, {frame: the values it encodes})"""
    import torch
    dev = torch.device("cuda:0")
    shape = (F_ALL, L) if fmt == "f32" else (F_ALL, L, 2)
    x = torch.full(shape, 128, device=dev, dtype=torch.uint8) if fmt == "cu8" else \
        torch.zeros(shape, device=dev, dtype=getattr(torch, TORCH_DT[fmt]))
    raw, vals = {}, {}
    for f, v in _source(zoom, L).items():
        raw[f], vals[f] = (np.ascontiguousarray(v), v) if fmt == "complex64" else _encode(v, fmt)
        flat = raw[f].view(np.float32) if fmt == "complex64" else np.ascontiguousarray(raw[f])
        x[f] = torch.from_numpy(flat.reshape(shape[1:])).to(dev)
    return x, raw, vals


def _rows(zoom, x, L, F, fmt, flip):
    import torch
    from pypanadapter_amd import ZoomFFT
    W = N // zoom
    rows = torch.empty((F, W), device=x.device, dtype=torch.float32)
    with ZoomFFT(N, zoom, 2.4e6, n_win=W, in_dtype=fmt, flip=flip) as plan:
        plan.set_path(6)
        plan.set_timing(True)
        plan.process_device(x.data_ptr(), L, F, rows.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        names = plan.launch_names()
    assert "fc_decim" in names, names
    return rows.cpu().numpy()


def test_shapes_walk_both_paths():
    assert _paths(L8, 8) == ["edge", "carried", "carried", "carried", "edge"]
    assert _paths(L4, 4).count("carried") >= 2
    assert _paths(L8, 8, bpc=3) == ["edge", "carried", "carried", "edge", "edge"]
    assert PICKS[1] + 1 == PICKS[2] and max(PICKS) < F_ALL // 2


@pytest.mark.parametrize("zoom,L,fmt,flip", CASES,
                         ids=[f"zoom{z}-{fmt}-{'flip' if fl else 'noflip'}" for z, _, fmt, fl in CASES])
def test_fc_prefetch_rows_and_iq_vs_oracle(oracle_lib, zoom, L, fmt, flip):
    from pypanadapter_amd import ZoomFFT
    x, raw, vals = _batch(zoom, L, fmt)
    got = _rows(zoom, x, L, F_ALL, fmt, flip)
    ref_in = {f: np.ascontiguousarray(v[::-1] if flip else v) for f, v in vals.items()}
    for f in PICKS:
        assert_row_close(got[f], oracle_lib.psd_row(ref_in[f], 2.4e6, N, zoom, N // zoom),
                         f"zoom {zoom} {fmt} flip={flip} frame {f}")
    # a zero frame right behind a picked one gives what every other zero frame gives
    np.testing.assert_array_equal(got[PICKS[2] + 1], got[100])
    with ZoomFFT(N, zoom, 2.4e6, n_win=N // zoom, in_dtype=fmt, flip=flip) as plan:
        plan.set_path(6)
        for f in PICKS[1:]:
            plan.set_timing(True)
            d = plan.decimate(raw[f])
            assert "fc_decim" in plan.launch_names(), plan.launch_names()
            ref = oracle_lib.zoomfft(ref_in[f], zoom, 2.4e6)
            assert d.shape == ref.shape, (d.shape, ref.shape)
            e = check_rel(d, ref, FC_TOL, f"fc_prefetch/zoom{zoom}/{fmt}", (flip, f))
            print(f"zoom {zoom} {fmt} flip={flip} frame {f}: IQ error {e:.3e} of the peak (bound {FC_TOL})")


@pytest.mark.parametrize("fmt,flip", [("complex64", True), ("cu8", False)], ids=["complex64-flip", "cu8"])
def test_fc_prefetch_run_boundary(oracle_lib, fmt, flip):
    """512 frames per call: a frame splits into two runs of blocks and block 3, carried in the
    1024-frame call, starts the second run on the edge path."""
    x, _, vals = _batch(8, L8, fmt)
    got = _rows(8, x, L8, F_ALL // 2, fmt, flip)
    for f in PICKS:
        ref_in = np.ascontiguousarray(vals[f][::-1] if flip else vals[f])
        assert_row_close(got[f], oracle_lib.psd_row(ref_in, 2.4e6, N, 8, N // 8), f"{fmt} frame {f}")
