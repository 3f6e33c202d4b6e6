"""CPU checks of the decimator schedule chooser (csrc/zfft_schedule.cpp, no GPU needed).

* TABLE pins choose_schedule through the zfft__schedule hook: every (zoom, in_dtype, path, L,
  frames) -> schedule name, or "unsupported" where the call is refused (ZFFT_EUNSUPPORTED).
  The names are written down from the fall-through chain the chooser replaced (run_decimator /
  run_pc / run_pc_head before the split); test_gpu_parity.test_auto_schedule_by_batch ties the
  hook to the launches that actually run.
* tests/host/schedule_sweep.cpp sweeps the chooser's whole domain for its invariants (domain
  limits of each kernel form, 64-bit products) under ASan + UBSan, as a stand-alone program.

in_dtype: 0 complex64 (8 B per sample), 1 complex32 (4), 2 cu8 (2), 3 real f32 (4)."""
import ctypes
import os
import shutil
import subprocess

import pytest

ZFFT_EUNSUPPORTED = -6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TABLE = [
    # auto
    (8, 0, 0, 299008, 1, "pc8_tiles"), (8, 0, 0, 299008, 15, "pc8_tiles"), (8, 0, 0, 299008, 16, "fc8"),
    (8, 0, 0, 299008, 384, "fc8"), (8, 0, 0, 1048576, 768, "fc8"), (8, 0, 0, 32768, 1024, "fc8"),
    (8, 0, 0, 32768, 1023, "fc8"), (8, 0, 0, 8192, 4, "exact"), (4, 0, 0, 262144, 1, "pc4_tiles"),
    (4, 0, 0, 262144, 31, "pc4_tiles"), (4, 0, 0, 262144, 32, "fc4"), (4, 0, 0, 262144, 256, "fc4"),
    (4, 0, 0, 262144, 384, "fc4"), (4, 0, 0, 1048576, 64, "fc4"), (4, 0, 0, 65536, 511, "fc4"),
    (4, 0, 0, 65536, 512, "fc4"), (4, 0, 0, 65536, 1024, "fc4"), (4, 0, 0, 8192, 768, "xa"),
    (2, 0, 0, 65536, 512, "xa"), (2, 0, 0, 65536, 511, "pc2_tiles"), (2, 0, 0, 262144, 8, "pc2_tiles"),
    (2, 0, 0, 1048576, 600, "pc2_tiles"), (2, 0, 0, 1048576, 768, "xa"), (2, 0, 0, 8192, 8, "exact"),
    (16, 0, 0, 262144, 384, "fc8+pc2_exact"), (16, 0, 0, 262144, 512, "fc8+xa"),
    (16, 0, 0, 262144, 8, "pc8_tiles+pc2_exact"),
    # batches
    (8, 0, 0, 32768, 512, "fc8"), (4, 0, 0, 32768, 1050, "fc4"), (2, 0, 0, 32768, 1050, "xa"),
    (2, 0, 0, 32768, 250, "pc2_tiles"), (4, 0, 0, 32768, 250, "fc4"), (4, 0, 0, 32768, 20, "pc4_tiles"),
    # thresholds
    (8, 0, 0, 524288, 15, "pc8_tiles"), (8, 0, 0, 524288, 16, "fc8"), (8, 0, 0, 524289, 15, "pc8_tiles"),
    (8, 0, 0, 524289, 16, "fc8"), (4, 0, 0, 524288, 31, "pc4_tiles"), (4, 0, 0, 524288, 32, "fc4"),
    (4, 0, 0, 524289, 31, "pc4_tiles"), (4, 0, 0, 524289, 32, "fc4"), (4, 0, 0, 268435456, 511, "pc4_tiles"),
    (4, 0, 0, 268435456, 512, "walk4"), (8, 0, 0, 268435456, 1023, "pc8_tiles"),
    (8, 0, 0, 268435456, 1024, "walk8"), (2, 0, 0, 524288, 383, "pc2_tiles"),
    (2, 0, 0, 524288, 384, "pc2_tiles"), (2, 0, 0, 524288, 511, "pc2_tiles"), (2, 0, 0, 524288, 512, "xa"),
    (2, 0, 0, 524288, 767, "xa"), (2, 0, 0, 524288, 768, "xa"), (2, 0, 0, 524289, 383, "pc2_tiles"),
    (2, 0, 0, 524289, 384, "pc2_tiles"), (2, 0, 0, 524289, 511, "pc2_tiles"),
    (2, 0, 0, 524289, 512, "pc2_tiles"), (2, 0, 0, 524289, 767, "pc2_tiles"), (2, 0, 0, 524289, 768, "xa"),
    (8, 0, 0, 8192, 383, "exact"), (8, 0, 0, 8192, 384, "xa"), (8, 0, 0, 8192, 767, "xa"),
    (8, 0, 0, 8192, 768, "xa"), (8, 0, 0, 16384, 65535, "fc8"), (8, 0, 0, 16384, 65536, "xa"),
    (8, 0, 0, 524289, 65536, "xa"),
    # min_L
    (2, 0, 0, 16383, 1, "exact"), (2, 0, 0, 16384, 1, "pc2_tiles"), (4, 0, 0, 16383, 1, "exact"),
    (4, 0, 0, 16384, 1, "pc4_tiles"), (8, 0, 0, 16383, 1, "exact"), (8, 0, 0, 16384, 1, "pc8_tiles"),
    (16, 0, 0, 16383, 1, "exact"), (16, 0, 0, 16384, 1, "pc8_tiles+pc2_exact"),
    # max_frames
    (2, 0, 0, 16384, 65535, "xa"), (2, 0, 0, 16384, 65536, "xa"), (2, 0, 4, 16384, 65535, "pc2_tiles"),
    (2, 0, 4, 16384, 65536, "unsupported"), (4, 0, 0, 16384, 65535, "fc4"), (4, 0, 0, 16384, 65536, "xa"),
    (4, 0, 4, 16384, 65535, "pc4_tiles"), (4, 0, 4, 16384, 65536, "unsupported"),
    (8, 0, 0, 16384, 65535, "fc8"), (8, 0, 0, 16384, 65536, "xa"), (8, 0, 4, 16384, 65535, "pc8_tiles"),
    (8, 0, 4, 16384, 65536, "unsupported"), (16, 0, 0, 16384, 65535, "fc8+xa"),
    (16, 0, 0, 16384, 65536, "xa"), (16, 0, 4, 16384, 65535, "pc8_tiles+xa"),
    (16, 0, 4, 16384, 65536, "unsupported"),
    # forced
    (2, 0, 1, 32768, 8, "exact"), (2, 0, 1, 8192, 8, "exact"), (2, 0, 2, 32768, 8, "exact"),
    (2, 0, 2, 8192, 8, "exact"), (2, 0, 3, 32768, 8, "xa"), (2, 0, 3, 8192, 8, "xa"),
    (2, 0, 4, 32768, 8, "pc2_tiles"), (2, 0, 4, 8192, 8, "unsupported"), (2, 0, 5, 32768, 8, "pc2_tiles"),
    (2, 0, 5, 8192, 8, "unsupported"), (2, 0, 6, 32768, 8, "pc2_tiles"), (2, 0, 6, 8192, 8, "unsupported"),
    (4, 0, 1, 32768, 8, "exact"), (4, 0, 1, 8192, 8, "exact"), (4, 0, 2, 32768, 8, "fused"),
    (4, 0, 2, 8192, 8, "exact"), (4, 0, 3, 32768, 8, "xa"), (4, 0, 3, 8192, 8, "xa"),
    (4, 0, 4, 32768, 8, "pc4_tiles"), (4, 0, 4, 8192, 8, "unsupported"), (4, 0, 5, 32768, 8, "walk4"),
    (4, 0, 5, 8192, 8, "unsupported"), (4, 0, 6, 32768, 8, "fc4"), (4, 0, 6, 8192, 8, "unsupported"),
    (8, 0, 1, 32768, 8, "exact"), (8, 0, 1, 8192, 8, "exact"), (8, 0, 2, 32768, 8, "exact"),
    (8, 0, 2, 8192, 8, "exact"), (8, 0, 3, 32768, 8, "xa"), (8, 0, 3, 8192, 8, "xa"),
    (8, 0, 4, 32768, 8, "pc8_tiles"), (8, 0, 4, 8192, 8, "unsupported"), (8, 0, 5, 32768, 8, "walk8"),
    (8, 0, 5, 8192, 8, "unsupported"), (8, 0, 6, 32768, 8, "fc8"), (8, 0, 6, 8192, 8, "unsupported"),
    (16, 0, 1, 32768, 8, "exact"), (16, 0, 1, 8192, 8, "exact"), (16, 0, 2, 32768, 8, "exact"),
    (16, 0, 2, 8192, 8, "exact"), (16, 0, 3, 32768, 8, "xa"), (16, 0, 3, 8192, 8, "xa"),
    (16, 0, 4, 32768, 8, "pc8_tiles+pc2_exact"), (16, 0, 4, 8192, 8, "unsupported"),
    (16, 0, 5, 32768, 8, "walk8+pc2_exact"), (16, 0, 5, 8192, 8, "unsupported"),
    (16, 0, 6, 32768, 8, "fc8+pc2_exact"), (16, 0, 6, 8192, 8, "unsupported"),
    # forced_never_pc
    (2, 0, 1, 1048576, 1024, "exact"), (2, 0, 2, 1048576, 1024, "exact"), (4, 0, 1, 1048576, 1024, "exact"),
    (4, 0, 2, 1048576, 1024, "fused"), (8, 0, 1, 1048576, 1024, "exact"), (8, 0, 2, 1048576, 1024, "fused"),
    (16, 0, 1, 1048576, 1024, "exact"), (16, 0, 2, 1048576, 1024, "fused"),
    # bytes
    (8, 0, 3, 268435455, 1, "xa"), (8, 0, 3, 268435456, 1, "unsupported"), (8, 0, 6, 268435455, 1, "fc8"),
    (8, 0, 6, 268435456, 1, "walk8"), (8, 0, 0, 268435455, 16, "fc8"), (8, 0, 0, 268435456, 16, "pc8_tiles"),
    (8, 0, 0, 268435455, 768, "fc8"), (8, 0, 0, 268435456, 768, "pc8_tiles"),
    (16, 0, 0, 268435455, 1, "pc8_tiles+pc2_exact"), (16, 0, 0, 268435456, 1, "fused"),
    (4, 0, 6, 268435455, 1, "fc4"), (4, 0, 6, 268435456, 1, "walk4"), (8, 2, 0, 1073741823, 16, "fc8"),
    (8, 2, 0, 1073741824, 16, "pc8_tiles"), (8, 2, 3, 1073741823, 1, "unsupported"),
    (8, 2, 3, 1073741824, 1, "unsupported"), (8, 2, 6, 1073741823, 1, "fc8"),
    (8, 2, 6, 1073741824, 1, "walk8"), (16, 2, 0, 1073741823, 16, "fused"),
    (16, 2, 0, 1073741824, 16, "fused"), (16, 2, 3, 1073741823, 1, "unsupported"),
    (16, 2, 3, 1073741824, 1, "unsupported"), (16, 2, 6, 1073741823, 1, "fc8+pc2_exact"),
    (16, 2, 6, 1073741824, 1, "walk8+pc2_exact"), (8, 2, 3, 268435455, 1, "xa"),
    (8, 2, 3, 268435456, 1, "unsupported"), (8, 1, 6, 536870911, 1, "fc8"), (8, 1, 6, 536870912, 1, "walk8"),
    (8, 3, 6, 536870911, 1, "fc8"), (8, 3, 6, 536870912, 1, "walk8"),
    # tail
    (16, 0, 0, 131064, 383, "fc8+pc2_exact"), (16, 0, 0, 131064, 384, "fc8+xa"),
    (16, 0, 0, 131064, 511, "fc8+xa"), (16, 0, 0, 131064, 512, "fc8+xa"),
    (16, 0, 0, 131072, 383, "fc8+pc2_exact"), (16, 0, 0, 131072, 384, "fc8+pc2_exact"),
    (16, 0, 0, 131072, 511, "fc8+pc2_exact"), (16, 0, 0, 131072, 512, "fc8+xa"),
    (16, 0, 0, 4194304, 383, "fc8+pc2_exact"), (16, 0, 0, 4194304, 384, "fc8+pc2_exact"),
    (16, 0, 0, 4194304, 511, "fc8+pc2_exact"), (16, 0, 0, 4194304, 512, "fc8+xa"),
    (16, 0, 0, 4194312, 383, "fc8+pc2_exact"), (16, 0, 0, 4194312, 384, "fc8+pc2_exact"),
    (16, 0, 0, 4194312, 511, "fc8+pc2_exact"), (16, 0, 0, 4194312, 512, "fc8+pc2_exact"),
    (64, 0, 0, 131064, 383, "fc8+pc2_exact"), (64, 0, 0, 131064, 384, "fc8+xa"),
    (64, 0, 0, 131064, 511, "fc8+xa"), (64, 0, 0, 131064, 512, "fc8+xa"),
    (64, 0, 0, 131072, 383, "fc8+pc2_exact"), (64, 0, 0, 131072, 384, "fc8+pc2_exact"),
    (64, 0, 0, 131072, 511, "fc8+pc2_exact"), (64, 0, 0, 131072, 512, "fc8+xa"),
    (64, 0, 0, 4194304, 383, "fc8+pc2_exact"), (64, 0, 0, 4194304, 384, "fc8+pc2_exact"),
    (64, 0, 0, 4194304, 511, "fc8+pc2_exact"), (64, 0, 0, 4194304, 512, "fc8+xa"),
    (64, 0, 0, 4194312, 383, "fc8+pc2_exact"), (64, 0, 0, 4194312, 384, "fc8+pc2_exact"),
    (64, 0, 0, 4194312, 511, "fc8+pc2_exact"), (64, 0, 0, 4194312, 512, "fc8+pc2_exact"),
]


def _hook():
    from pypanadapter_amd import _lib as L, build
    build.build()
    f = L.load().zfft__schedule
    f.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32,
                  ctypes.c_char_p, ctypes.c_int32]
    f.restype = ctypes.c_int
    return f


def schedule(zoom, in_dtype, path, L, frames):
    """(rc, name) of zfft__schedule."""
    buf = ctypes.create_string_buffer(32)
    rc = _hook()(zoom, in_dtype, path, L, frames, buf, len(buf))
    return rc, buf.value.decode()


def test_schedule_table():
    assert len(set(TABLE)) == len({t[:5] for t in TABLE})  # no key with two answers
    wrong = []
    for zoom, dt, path, L, frames, want in TABLE:
        rc, name = schedule(zoom, dt, path, L, frames)
        if name != want or rc != (ZFFT_EUNSUPPORTED if want == "unsupported" else 0):
            wrong.append(((zoom, dt, path, L, frames), want, name, rc))
    assert not wrong, wrong


def test_schedule_hook_arguments():
    assert schedule(1, 0, 0, 4096, 1) == (0, "none")  # zoom 1: no decimator
    assert schedule(3, 0, 0, 65536, 1)[0] == -1       # ZFFT_EINVAL: zoom not a power of two
    assert schedule(8, 4, 0, 65536, 1)[0] == -1       # unknown in_dtype
    buf = ctypes.create_string_buffer(4)              # a short buffer truncates, terminated
    assert _hook()(16, 0, 0, 262144, 512, buf, 4) == 0 and buf.value == b"fc8"


def test_schedule_sweep_sanitized(tmp_path):
    """The chooser over its whole domain as a stand-alone g++ program (no HIP, no Python in the
    child) under AddressSanitizer + UBSan: the invariants in tests/host/schedule_sweep.cpp."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/host/schedule_sweep.cpp"
    csrc = os.path.join(ROOT, "pypanadapter_amd", "csrc")
    exe = str(tmp_path / "schedule_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", csrc, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "schedule_sweep.cpp"),
                    os.path.join(csrc, "zfft_schedule.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "schedule_sweep: ok" in r.stdout, r.stdout
