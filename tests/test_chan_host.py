"""CPU checks of the channeliser's host side: the form chooser through its hook over a grid (spans
are whole steps, cover the push exactly, LDS within the limit) and, over its whole domain, as a
stand-alone program under ASan + UBSan (tests/host/chan_form_sweep.cpp); the step counts against
the reference; the default prototype against tap_design; the C-ABI's new names, their ctypes
signatures and the errors that need no device; and the reference itself against the tap
reference, channel by channel."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import chan_ref as cr
import tap_ref as tp
from test_host import header_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["zfft_plan_chan", "zfft_chan_shape", "zfft_chan_select", "zfft_chan_steps", "zfft_chan_push_device",
         "zfft_chan_push", "zfft_chan_state", "zfft_chan_reset", "zfft_chan_info", "zfft_chan_design"]
EINVAL = -1
FORM = ("span", "steps_per_span", "points", "halo", "kind", "radix1", "passes", "lds_bytes", "grid", "r0", "odd0",
        "nspans", "steps")


def chan_form(lib, n0, n, M, P, D, K=None):
    """The form dict of zfft__chan_form, or None where it refuses."""
    hook = lib.zfft__chan_form
    hook.argtypes = [ctypes.c_uint64, ctypes.c_int64] + [ctypes.c_int32] * 4 + [ctypes.c_void_p]
    hook.restype = ctypes.c_int
    form = np.zeros(len(FORM), np.int64)
    if hook(n0, n, M, P, D, M if K is None else K, form.ctypes.data_as(ctypes.c_void_p)):
        return None
    return dict(zip(FORM, map(int, form)))


def test_form_chooser_through_the_hook(zfft_lib):
    shapes = cr.CASES + [(8, 256, 8), (512, 4, 256), (1024, 2, 1024), (64, 8, 64), (64, 32, 32)]
    for M, P, D in shapes:
        T = M * P
        for n0 in (0, 5, D - 1, D, 2 ** 32 - 100, 2 ** 40 + 3):
            for n in (1, D - 1, D, T - 1, 3000, 5000, 65536, 524289, 4096 * 299008, 2 ** 31 - 1):
                for K in (1, M // 2 + 1, M):
                    f = chan_form(zfft_lib, n0, n, M, P, D, K)
                    assert f is not None, (M, P, D, n0, n, K)
                    S = f["steps_per_span"]
                    assert f["points"] in (1024, 2048, 4096) and S * M == f["points"]
                    assert f["span"] == S * D                                   # whole steps
                    assert f["nspans"] == -(-n // f["span"])                     # every sample in exactly one span
                    assert f["grid"] == min(f["nspans"], 1024)
                    assert f["halo"] == T - 1 and f["kind"] == (0 if P <= 8 else 1)
                    assert f["lds_bytes"] == 8 * (f["halo"] + f["span"] + f["points"] + M) + 4 * K + (4 * T if P > 8 else 0)
                    assert f["lds_bytes"] <= 64 * 1024                           # no attribute, two workgroups a CU
                    assert f["radix1"] == (8 if int(np.log2(M)) & 1 else 4)
                    assert f["radix1"] * 4 ** (f["passes"] - 1) == M
                    assert 0 <= f["r0"] < D and (n0 + f["r0"]) % D == 0
                    assert f["odd0"] == ((cr.ceil_div(n0, D) & 1) if D != M else 0)
                    assert f["steps"] == cr.steps(n0, n, D)
                    assert f["points"] == 1024 or f["nspans"] >= 512
    # the cases the GPU tests name: a few thousand samples run at the shortest span
    assert chan_form(zfft_lib, 0, 5000, 64, 8, 32)["span"] == 16 * 32
    assert chan_form(zfft_lib, 0, 5000, 1024, 2, 512)["span"] == 512
    assert chan_form(zfft_lib, 0, 4096 * 299008, 64, 8, 32)["span"] == 64 * 32
    for bad in [(0, 0, 64, 8, 32), (0, 2 ** 31, 64, 8, 32), (2 ** 62 + 1, 10, 64, 8, 32), (0, 10, 48, 8, 24),
                (0, 10, 4, 8, 4), (0, 10, 2048, 1, 2048), (0, 10, 64, 0, 32), (0, 10, 64, 33, 32), (0, 10, 64, 8, 16),
                (0, 10, 64, 8, 63), (0, 10, 64, 8, 32, 0), (0, 10, 64, 8, 32, 65)]:
        assert chan_form(zfft_lib, *bad) is None, bad
    pos = zfft_lib.zfft__chan_position
    pos.argtypes, pos.restype = [ctypes.c_int32, ctypes.c_int32], ctypes.c_int
    for M in (8, 16, 32, 64, 128, 256, 512, 1024):
        assert sorted(pos(M, c) for c in range(M)) == list(range(M))
    assert pos(8, 8) == -1 and pos(12, 0) == -1


def test_step_counts_are_the_reference(zfft_lib):
    hook = zfft_lib.zfft__chan_steps
    hook.argtypes, hook.restype = [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int32], ctypes.c_int64
    for n0 in (0, 1, 7, 511, 512, 4096, 2 ** 32 - 100, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 3, 2 ** 62 - 2 ** 31):
        for D in (4, 8, 32, 64, 512, 1024):
            for n in (0, 1, 2, D - 1, D, D + 1, 1023, 5000, 2 ** 31 - 1):
                assert hook(n0, n, D) == cr.steps(n0, n, D) == len(range(cr.ceil_div(n0, D), cr.ceil_div(n0 + n, D)))
    # cutting a stretch never changes the total
    for n0, D in ((2 ** 32 - 100, 32), (2 ** 40 + 3, 512), (5, 8)):
        cuts = [1, 1, 7, D - 1, 64, 63, 1023, 4000]
        at, total = n0, 0
        for n in cuts:
            total += hook(at, n, D)
            at += n
        assert total == hook(n0, sum(cuts), D) == cr.steps(n0, sum(cuts), D)


def test_design_is_the_tap_design(zfft_lib):
    from pypanadapter_amd.engine import chan_design, tap_design
    for M, P, beta in [(8, 1, 8.0), (8, 8, 8.0), (64, 8, 8.0), (64, 8, 5.0), (1024, 2, 8.0), (16, 128, 10.0)]:
        h = chan_design(M, P, beta)
        assert h.dtype == np.float64 and h.shape == (M * P,)
        assert np.array_equal(h, tap_design(M * P, 0.5 / M, beta))
        assert abs(h.sum() - 1.0) <= 1e-12
    # -6 dB at the channel edge: |H(0.5 / M)| = 1/2 of the DC gain (a windowed sinc's cutoff)
    h = chan_design(64, 8)
    edge = abs(np.sum(h * np.exp(-2j * np.pi * (0.5 / 64) * np.arange(h.size))))
    assert abs(edge - 0.5) <= 2e-3
    for bad in [(0, 8, 8.0), (12, 8, 8.0), (4, 8, 8.0), (2048, 1, 8.0), (64, 0, 8.0), (64, 33, 8.0), (64, 8, -1.0)]:
        with pytest.raises(ValueError):
            chan_design(*bad)
    assert zfft_lib.zfft_chan_design(8, 8, 8.0, None) == EINVAL


def test_chan_form_sweep_sanitized(tmp_path):
    """The chooser, the counts, the positions and the twiddles over their domain as a stand-alone g++
    program (no HIP, no Python in the child) under AddressSanitizer + UBSan: tests/host/chan_form_sweep.cpp."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/host/chan_form_sweep.cpp"
    csrc = os.path.join(ROOT, "pypanadapter_amd", "csrc")
    exe = str(tmp_path / "chan_form_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", csrc, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "chan_form_sweep.cpp"),
                    os.path.join(csrc, "zfft_chan_plan.cpp"), os.path.join(csrc, "zfft_tap_plan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "chan_form_sweep: ok" in r.stdout, r.stdout


def test_new_names_signatures_and_null_plan_errors(zfft_lib):
    from pypanadapter_amd import _lib
    import pypanadapter_amd as pkg
    declared = header_functions()
    for name in NAMES:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert getattr(zfft_lib, name).argtypes is not None and getattr(zfft_lib, name).restype is ctypes.c_int, name
    I32, I64, P = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    assert zfft_lib.zfft_plan_chan.argtypes == [P, I32, I32, I32, P]
    assert zfft_lib.zfft_chan_select.argtypes == [P, I32, I32]
    assert zfft_lib.zfft_chan_push_device.argtypes == [P, P, I64, P, P]
    assert zfft_lib.zfft_chan_push.argtypes == [P, P, I64, P, P]
    assert zfft_lib.zfft_chan_reset.argtypes == [P, I64]
    assert zfft_lib.zfft_chan_design.argtypes == [I32, I32, ctypes.c_double, P]
    for name in ("set_channels", "chan_shape", "chan_select", "chan_steps", "chan_push", "chan_push_device", "chan_state",
                 "chan_reset", "chan_info", "chan_freqs"):
        assert callable(getattr(pkg.ZoomFFT, name)), name
    assert callable(pkg.chan_design) and isinstance(pkg.Channelizer, type)
    # a null plan is EINVAL before anything touches a device
    v32, v64, u64, dbl = I32(), I64(), ctypes.c_uint64(), ctypes.c_double()
    h = np.float32([1.0] * 8)
    hp = h.ctypes.data_as(P)
    r = ctypes.byref
    assert zfft_lib.zfft_plan_chan(None, 8, 1, 8, hp) == EINVAL
    assert zfft_lib.zfft_chan_shape(None, r(v32), r(v32), r(v32), r(v32), r(v32)) == EINVAL
    assert zfft_lib.zfft_chan_select(None, 0, 8) == EINVAL
    assert zfft_lib.zfft_chan_steps(None, 5, r(v64)) == EINVAL
    assert zfft_lib.zfft_chan_push_device(None, hp, 1, hp, None) == EINVAL
    assert zfft_lib.zfft_chan_push(None, hp, 1, hp, None) == EINVAL
    assert zfft_lib.zfft_chan_state(None, r(u64)) == EINVAL
    assert zfft_lib.zfft_chan_reset(None, 0) == EINVAL
    assert zfft_lib.zfft_chan_info(None, r(dbl), r(dbl)) == EINVAL
    text = open(os.path.join(ROOT, "include", "zfft.h")).read()
    rule = text[text.index("/* Channeliser:"):text.index("int zfft_plan_chan(")]
    for clause in ("bit for bit", "T - 1", "(P + 5 log2 M + 2) 2^-24", "k ascending", "ZFFT_EUNSUPPORTED", "DFT_M",
                   "channels are off", "chan_push"):
        assert clause in rule, clause


def test_the_reference_is_the_tap_reference_channel_by_channel():
    """The bank's rule is a tap at freq_word c 2^32 / M on the same count: chan_ref against tap_ref,
    float64 both, and chan_ref's own invariance under cutting (the property the carry has to keep)."""
    rng = np.random.default_rng(1)
    for M, P, D, n0 in [(8, 3, 8, 0), (8, 3, 4, 5), (16, 4, 8, 2 ** 32 - 37), (16, 2, 16, 2 ** 40 + 3)]:
        h = rng.standard_normal(M * P).astype(np.float32)
        x = tp.noise_and_tones(5 * M + 3, 3).astype(np.complex128)
        ms = cr.step_indices(n0, x.size, D)
        assert len(ms) == cr.steps(n0, x.size, D) == tp.count(n0, n0, x.size, D)
        y = cr.ref_chan(x, n0, M, D, h, ms)
        for c in range(M):
            fw = (c * 2 ** 32 // M + 2 ** 31) % 2 ** 32 - 2 ** 31
            want = tp.ref_tap(x, n0, fw, D, h, np.array(ms, dtype=np.int64))
            assert np.abs(want - y[:, c]).max() <= 1e-13, (M, P, D, n0, c)
        late = ms[-1:]
        a = late[0] * D - n0 - (M * P - 1)
        assert a >= 0
        part = cr.ref_chan(x[a:], n0 + a, M, D, h, late)
        assert np.array_equal(part, y[len(ms) - len(late):])
