"""Shapes, inputs and the run of tests/test_gpu_fc_tail.py, shared by the test and by the child
process that runs the same cases on a FC_TAIL_CARRY=0 build of the library (a process loads one
libzfft.so: ZFFT_LIB_PATH selects it).  As a program:
    python tests/fc_tail_cases.py OUT.json      digests of every case's decimated IQ"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 2.4e6
HOP = {8: 6656, 4: 7168}
# Frame lengths against the window grid (a window is 8192 samples, K = 768 / 512 of them before the
# block's first output).  Zoom 8, by what the frame's end does to the last windows:
#   8192 + 6656 - 768 = 14,080: the second window ends with the frame and the third, last one
#   keeps 1536 samples of it; - 1: the second window's last pair is half outside; + 1 and + 7:
#   the other side, odd (a pair across the end) and L mod 8 = 7; 13,313 = 2 x 6656 + 1: the
#   last window keeps 769 samples, all in pairs it carries, so every new request of it lies past
#   the frame; 20,737: one hop more than 14,081.
# The schedule gives FC (path 6) only frames of >= 16,384 samples (the frame-end maps beside it
# need them), so each length is taken one hop longer: the same position against the grid, one
# carried block more.  Zoom 4: the same positions on its grid (hop 7168, K = 512).
LENGTHS = {8: [L + 6656 for L in (14079, 14080, 14081, 14087, 13313, 20737)],
           4: [L + 7168 for L in (14847, 14848, 14849, 14851, 14337, 22017)]}
FORMATS = ("complex64", "complex32", "f32")
# 1024 frames per call: one workgroup walks a whole frame; 512: runs of two blocks
FRAMES = (1024, 512)
PICKS = (0, 317, -1)                    # frames compared with the oracle
LMAX = max(max(v) for v in LENGTHS.values())


def base_input():
    """(1024, LMAX) complex64, made once: noise and a tone per frame, below full scale for float16."""
    rng = np.random.default_rng(9100)
    x = rng.standard_normal((max(FRAMES), 2 * LMAX), dtype=np.float32).view(np.complex64)
    x *= np.float32(0.25)
    n = np.arange(LMAX, dtype=np.float64)
    tones = np.exp(2j * np.pi * (0.0009 + 0.0013 * np.arange(7))[:, None] * n[None, :]).astype(np.complex64)
    for k in range(7):
        x[k::7] += tones[k]
    return x


def encode(x, fmt):
    """The plan's input array and the values it stands for (what the oracle is given)."""
    if fmt == "complex64":
        return np.ascontiguousarray(x), x
    if fmt == "complex32":
        h = np.ascontiguousarray(x).view(np.float32).astype(np.float16)
        return h, h.astype(np.float32).view(np.complex64)
    r = np.ascontiguousarray(x.real)
    return r, r


def run_case(base, zoom, fmt, F, L):
    """Decimated IQ (F, m) of path 6 and the values of the picked frames."""
    from pypanadapter_amd import ZoomFFT
    arr, vals = encode(base[:F, :L], fmt)
    with ZoomFFT(1024, zoom, FS, in_dtype=fmt) as plan:
        plan.set_path(6)
        plan.set_timing(True)
        d = plan.decimate_frames(arr)
        names = plan.launch_names()
    assert names[0] == "fc_decim", names
    return d, {f: np.asarray(vals[f]) for f in PICKS}


def digest(d):
    return hashlib.sha256(np.ascontiguousarray(d).view(np.uint8)).hexdigest()


def key(zoom, fmt, F, L):
    return f"{zoom}/{fmt}/{F}/{L}"


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    base = base_input()
    out = {}
    for zoom in LENGTHS:
        for fmt in FORMATS:
            for F in FRAMES:
                for L in LENGTHS[zoom]:
                    out[key(zoom, fmt, F, L)] = digest(run_case(base, zoom, fmt, F, L)[0])
    with open(sys.argv[1], "w") as fh:
        json.dump(out, fh)
