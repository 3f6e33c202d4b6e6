"""GPU check of the FC decimator's range-checked window requests (FC_TAIL_CARRY,
fc_prefetch_plan.h): with them every block after a run's first takes its window from
the registers and the prefetch, the frame's last, overhanging window included, whose pairs past
the frame's end come back 0 from the buffer range check instead of from a reload.

The decimated IQ of path 6 at batches that carry -- 1024 frames per call (one workgroup walks a
whole frame) and 512 (runs of two blocks); with few frames every block is a run's first and loads
in full -- for complex64, complex32 and real f32 at zoom 8 and 4, at frame lengths that put the
frame's end at every kind of position against the last windows (tests/fc_tail_cases.py):
  * picked frames against the float64 oracle at path 6's documented gate (test_gpu_fc.FC_TOL);
  * every frame bit for bit against a FC_TAIL_CARRY=0 build of the same sources (the code of
    before: one resource per frame, the last window reloaded), run in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fc_tail_cases as cases
from conftest import check_rel
from test_gpu_fc import FC_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu(zfft_lib):
    from pypanadapter_amd import device_count
    assert device_count() >= 1, "GPU tests need a HIP device"


@pytest.fixture(scope="module")
def base():
    x = cases.base_input()
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def knob0_digests(zfft_lib, tmp_path_factory):
    """Every case on the FC_TAIL_CARRY=0 build: built through build(defines=...) beside the shipped
    library (kept while the sources it was built from are the tree's), run once in a child."""
    from pypanadapter_amd import build
    lib = os.path.join(build.LIB_DIR, "variants", "libzfft_tail_carry0.so")
    stamp = lib + ".json"
    want = {"source_hash": build.source_hash(), "arch": build.ARCH, "defines": ["FC_TAIL_CARRY=0"]}
    try:
        with open(stamp) as fh:
            fresh = os.path.exists(lib) and json.load(fh) == want
    except (OSError, ValueError):
        fresh = False
    if not fresh:
        build.build(out=lib, defines=("FC_TAIL_CARRY=0",))
        with open(stamp, "w") as fh:
            json.dump(want, fh)
    out = str(tmp_path_factory.mktemp("fc_tail") / "knob0.json")
    env = dict(os.environ, ZFFT_LIB_PATH=lib)
    r = subprocess.run([sys.executable, os.path.join(cases.ROOT, "tests", "fc_tail_cases.py"), out],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with open(out) as fh:
        return json.load(fh)


def test_cases_put_the_frames_end_where_they_say():
    """The lengths against the block geometry (no GPU work): blocks per frame, and what is left
    of the frame for the last window."""
    for zoom, S, K in ((8, 13, 768), (4, 14, 512)):
        hop, P = 512 * S, 512 * S // zoom
        left = []
        for L in cases.LENGTHS[zoom]:
            assert L >= 16384
            nb = -(-(-(-L // zoom)) // P)
            left.append((nb, L - (hop * (nb - 1) - K)))
        assert [nb for nb, _ in left] == [4, 4, 4, 4, 4, 5], left
        # the last window keeps 2 K samples when the one before it ends with the frame; one less,
        # one more (odd: a pair across the end) and 7 (zoom 4: 3) more; K + 1 when the frame is
        # one sample longer than whole hops: every new request of the last window past the frame
        assert [n for _, n in left] == [2 * K - 1, 2 * K, 2 * K + 1, 2 * K + (7 if zoom == 8 else 3),
                                        K + 1, 2 * K + 1], left


@pytest.mark.parametrize("F", cases.FRAMES)
@pytest.mark.parametrize("fmt", cases.FORMATS)
@pytest.mark.parametrize("zoom", [8, 4])
def test_fc_tail_decimate(oracle_lib, base, knob0_digests, zoom, fmt, F):
    for L in cases.LENGTHS[zoom]:
        d, vals = cases.run_case(base, zoom, fmt, F, L)
        assert d.shape == (F, -(-L // zoom)), (L, d.shape)
        for f, v in vals.items():
            ref = oracle_lib.zoomfft(np.ascontiguousarray(v).astype(np.complex128), zoom, cases.FS)
            e = check_rel(d[f], ref, FC_TOL, f"fc{zoom}/tail/{fmt}", (L, F, f))
            print(f"zoom {zoom} {fmt} F={F} L={L} frame {f}: {e:.3e}")
        assert cases.digest(d) == knob0_digests[cases.key(zoom, fmt, F, L)], (zoom, fmt, F, L)
