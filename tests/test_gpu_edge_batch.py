"""GPU parity of the batched frame-end kernel behind the walk and FC (pc_edge_batch_kernel,
pc_kernels.hip): one workgroup makes both maps of four frames' ends on one side, so
what can go wrong is the tiling -- a last workgroup with fewer frames, LO rows that change inside
a workgroup, a frame's sums depending on its neighbours.

The decimated IQ, obtained as tests/test_gpu_fc.py obtains it, against the float64 oracle at that
file's FC_TOL (test_gpu_pc.PC_TOL for the walk), on the first and last 192 samples of every frame
(192 is the most outputs a frame-end map corrects).  Shapes are the smallest that tile: frames of
16384 and 20003 samples (L mod 8 = 0 and 3: different maps at the two ends), 1, 3, 5 and 18
frames per call (remainders 1, 3, 1 and 2 at four frames per workgroup)."""
import functools

import numpy as np
import pytest

from test_gpu_fc import FC_TOL
from test_gpu_pc import PC_TOL, _encode

pytestmark = pytest.mark.gpu
FS, N, EDGE, FMAX = 2.4e6, 1024, 192, 18
KERNEL = {5: "pc_walk", 6: "fc_decim"}


@pytest.fixture(scope="module", autouse=True)
def _gpu(zfft_lib):
    from pypanadapter_amd import device_count
    assert device_count() >= 1, "GPU tests need a HIP device"


@functools.lru_cache(maxsize=None)
def _input(L, f_lo=(1.0,)):
    """FMAX frames of noise plus a carrier each; read-only, shared by every case at this L and LO
    list.  The carrier sits 0.0071 fs above the LO that frame f is mixed with
    (f_lo[(f // 2) % len(f_lo)]: two frames per LO row), inside the passband, as synth.make_iq
    places its content in tests/test_gpu_fc.py.  A carrier left at 0.0071 fs under a 150 kHz LO
    lands at -133 kHz, on the filter's transition band, where it is a full-scale input that
    the output peak no longer shows: FC's error against that peak is then 0.9e-6 ... 1.2e-6 over
    the whole frame, the middle included, in the parent commit's library to the same digits
    (profiles/edge_batch/lo_offset_inputs.txt; DESIGN §3.9.2 is about such carriers), which says
    nothing about the frame ends."""
    rng = np.random.default_rng(9100 + L)
    x = (rng.standard_normal((FMAX, L)) + 1j * rng.standard_normal((FMAX, L))).astype(np.complex64)
    for f in range(FMAX):
        fc = f_lo[(f // 2) % len(f_lo)] / FS + 0.0071
        x[f] += np.exp(2j * np.pi * fc * np.arange(L)).astype(np.complex64)
    x.setflags(write=False)
    return x


_REFS = {}


def _ref(oracle_lib, key, frame, zoom, f_lo=1.0):
    """The oracle's decimated IQ of one frame, computed once per key."""
    if key not in _REFS:
        r = oracle_lib.zoomfft(np.ascontiguousarray(frame), zoom, FS, f_lo=f_lo)
        r.setflags(write=False)
        _REFS[key] = r
    return _REFS[key]


def _decimate(arr, zoom, path, **kw):
    from pypanadapter_amd import ZoomFFT
    with ZoomFFT(N, zoom, FS, **kw) as plan:
        plan.set_path(path)
        plan.set_timing(True)
        d = plan.decimate_frames(arr)
        names = plan.launch_names()
    assert KERNEL[path] in names and names.count("pc_edge") == 1, names
    return d


def _check_ends(d, ref, tol, what):
    """Both ends of one frame, relative to the frame's output peak (conftest.check_rel's measure)."""
    assert d.shape == ref.shape, (what, d.shape, ref.shape)
    err = np.abs(d - ref) / np.abs(ref).max()
    e = float(max(err[:EDGE].max(), err[-EDGE:].max()))
    print(f"{what}: ends {e:.3e} (bound {tol:.1e})")
    assert e < tol, (what, e)


@pytest.mark.parametrize("F", [1, 3, 5, 18])
@pytest.mark.parametrize("L", [16384, 20003])
@pytest.mark.parametrize("zoom,path", [(8, 6), (4, 6), (8, 5)], ids=["fc8", "fc4", "walk8"])
def test_frame_ends_vs_oracle(oracle_lib, zoom, path, L, F):
    x = _input(L)[:F]
    d = _decimate(x, zoom, path)
    assert d.shape[0] == F
    tol = FC_TOL if path == 6 else PC_TOL
    for f in range(F):
        _check_ends(d[f], _ref(oracle_lib, (zoom, L, f), x[f], zoom), tol, f"zoom {zoom} path {path} L {L} frame {f}/{F}")


def test_flip(oracle_lib):
    L, F = 20003, 5
    x = _input(L)[:F]
    d = _decimate(x, 8, 6, flip=True)
    for f in range(F):
        _check_ends(d[f], _ref(oracle_lib, ("flip", f), x[f, ::-1], 8), FC_TOL, f"flip frame {f}")


@pytest.mark.parametrize("fmt", ["complex32", "cu8", "f32"])
def test_input_formats(oracle_lib, fmt):
    L, F = 20003, 5
    arr, vals = _encode(_input(L)[:F], fmt)
    d = _decimate(arr, 8, 6, in_dtype=fmt)
    for f in range(F):
        _check_ends(d[f], _ref(oracle_lib, (fmt, f), vals[f], 8), FC_TOL, f"{fmt} frame {f}")


def test_lo_rows_change_inside_a_workgroup(oracle_lib):
    """Three LO rows, two frames each: frames 0-3 share a workgroup and use rows 0, 0, 1, 1;
    frame 4 (row 2) is alone in the last one."""
    from pypanadapter_amd import ZoomFFT
    L, F = 20003, 5
    f_lo = (1.0, 150e3 + 1.0, -300e3 + 1.0)
    x = _input(L, f_lo)[:F]
    with ZoomFFT(N, 8, FS) as plan:
        plan.set_path(6)
        plan.set_lo_frames(f_lo, 2)
        d = plan.decimate_frames(x)
    for f in range(F):
        lo = f_lo[(f // 2) % 3]
        _check_ends(d[f], _ref(oracle_lib, ("lo", lo, f), x[f], 8, f_lo=lo), FC_TOL, f"LO row {f // 2} frame {f}")


def test_lo_offset(oracle_lib):
    L, F, lo = 16384, 3, 150e3 + 1.0
    x = _input(L, (lo,))[:F]
    d = _decimate(x, 8, 6, f_lo=lo)
    for f in range(F):
        _check_ends(d[f], _ref(oracle_lib, ("lo", L, lo, f), x[f], 8, f_lo=lo), FC_TOL, f"f_lo frame {f}")


@pytest.mark.parametrize("zoom,path", [(8, 6), (4, 6), (8, 5)], ids=["fc8", "fc4", "walk8"])
def test_a_frame_does_not_depend_on_its_place(zoom, path):
    """Frame k of a 5-frame call equals, bit for bit, the same frame in a call of its own: a
    frame's sums do not depend on the workgroup's other frames or on its slot in the workgroup."""
    x = _input(20003)[:5]
    batch = _decimate(x, zoom, path)
    for k in range(5):
        np.testing.assert_array_equal(batch[k], _decimate(x[k:k + 1], zoom, path)[0], err_msg=f"frame {k}")
