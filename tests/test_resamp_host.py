"""CPU checks of the resampler bank's host side: the reference against scipy.signal.upfirdn and its
own invariance under cutting; the output count against Python integers where a 64-bit product
overflows; the design against the formula in numpy and its stated properties, recomputed; the
float32 model inside rule 7's gate; the form chooser through its hook over a grid and, over its
whole domain, as a stand-alone program under ASan + UBSan (tests/host/resamp_form_sweep.cpp); the
C-ABI's new names, their ctypes signatures and the errors that need no device."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.signal

import resamp_ref as rr
from test_host import header_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["zfft_plan_resamp", "zfft_resamp_shape", "zfft_resamp_steps", "zfft_resamp_push_device", "zfft_resamp_push",
         "zfft_resamp_state", "zfft_resamp_reset", "zfft_resamp_info", "zfft_resamp_design"]
EINVAL = -1
FORM = ("kind", "lanes", "span", "halo", "outs", "pitch", "lds_bytes", "lane_tiles", "nspans", "ntiles", "outputs", "p0",
        "grid")
# what DESIGN.md §3.3.12 states of the default design, for rr.DESIGN_RATIOS
RIPPLE_DB, STOP_DB, PHASE_GAIN = 0.003, 70.0, 1e-4


def resamp_form(lib, K, L, M, T, step_stride=None, fmt=0, n0=0, steps=1):
    """The form dict of zfft__resamp_form (the shape's form and the cut of a push), or None where it
    refuses."""
    hook = lib.zfft__resamp_form
    hook.argtypes = [ctypes.c_int32] * 4 + [ctypes.c_int64, ctypes.c_int32, ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p]
    hook.restype = ctypes.c_int
    form = np.zeros(len(FORM), np.int64)
    if hook(K, L, M, T, K if step_stride is None else step_stride, fmt, n0, steps, form.ctypes.data_as(ctypes.c_void_p)):
        return None
    return dict(zip(FORM, map(int, form)))


def lib_steps(lib, n0, steps, L, M):
    hook = lib.zfft__resamp_steps
    hook.argtypes, hook.restype = [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32], ctypes.c_int64
    return int(hook(n0, steps, L, M))


# ---------------------------------------------------------------- the reference
RATIOS9 = [(1, 1, 1), (3, 4, 8), (160, 147, 16), (2, 1, 5), (1, 7, 24), (5, 3, 1), (16, 25, 32), (147, 250, 32), (64, 25, 16)]


def test_reference_is_upfirdn_on_an_absolute_axis():
    x = np.random.default_rng(0).standard_normal((700, 2))
    for L, M, T in RATIOS9:
        h = rr.solid_taps(L, T).astype(np.float64)
        y = rr.ref_push(x, 0, h, L, M)
        assert y.shape == (rr.steps(0, len(x), L, M), 2)
        u = scipy.signal.upfirdn(h, x, L, M, axis=0)[:len(y)]
        assert np.abs(y - u).max() <= 1e-12, (L, M, T)


def test_reference_does_not_depend_on_the_cut():
    rng = np.random.default_rng(1)
    for L, M, T in [(3, 4, 8), (160, 147, 16), (1, 7, 24), (5, 3, 1)]:
        h = rr.solid_taps(L, T).astype(np.float64)
        x = rng.standard_normal((400, 3))
        for n0 in (0, 2 ** 32 - 100, 2 ** 40 + 3):
            whole = rr.ref_push(x, n0, h, L, M)
            for cut in (1, max(T - 1, 1), T, None):
                at, parts = 0, []
                while at < len(x):
                    c = int(rng.integers(1, 60)) if cut is None else cut
                    c = min(c, len(x) - at)
                    lo = max(0, at - (T - 1))             # the carry: T - 1 steps before the cut
                    parts.append(rr.ref_resamp(x[lo:at + c], n0 + lo, h, L, M, rr.out_indices(n0 + at, c, L, M)))
                    at += c
                got = np.concatenate(parts)
                assert got.shape == whole.shape and np.array_equal(got, whole), (L, M, T, n0, cut)


# ---------------------------------------------------------------- the count
def test_the_count_is_128_bits_wide(zfft_lib):
    L, M = 147, 250
    bites = 0
    for base in (2 ** 32, 2 ** 40, 2 ** 62 - 1000):
        for n0 in range(base - 3, base + 4):
            for n in (0, 1, 2, 249, 250, 251, 999):
                if n0 + n > 2 ** 62:
                    continue
                want = rr.steps(n0, n, L, M)
                assert lib_steps(zfft_lib, n0, n, L, M) == want, (n0, n)
                wrapped = -(-(((n0 + n) * L) % 2 ** 64) // M) - -(-((n0 * L) % 2 ** 64) // M)   # a 64-bit n0 L
                bites += wrapped != want
    assert bites > 0                                      # the case bites: 64 bits would differ at 2^62 - 1000
    assert (2 ** 62 - 1000) * L >= 2 ** 64
    rng = np.random.default_rng(2)
    for L, M in [(147, 250), (160, 147), (1, 4096), (512, 1), (16, 25)]:
        for n0 in (0, 2 ** 32 - 100, 2 ** 40 + 3, 2 ** 62 - 10 ** 6):
            cuts = [int(c) for c in rng.integers(0, 3000, 40)]
            at, total = n0, 0
            for c in cuts:
                total += lib_steps(zfft_lib, at, c, L, M)
                at += c
            assert total == lib_steps(zfft_lib, n0, sum(cuts), L, M) == rr.steps(n0, sum(cuts), L, M)
    for bad in [(0, -1, 3, 4), (0, 2 ** 31, 3, 4), (2 ** 62 + 1, 5, 3, 4), (0, 5, 2, 4), (0, 5, 0, 4), (0, 5, 3, 0), (0, 5, 513, 4),
                (0, 5, 3, 4097)]:
        assert lib_steps(zfft_lib, *bad) == 0, bad


# ---------------------------------------------------------------- the design
def test_design_is_the_formula_and_has_its_stated_properties(zfft_lib):
    from pypanadapter_amd import resamp_design
    for L, M in rr.DESIGN_RATIOS:
        T = rr.default_taps_per_phase(L, M)
        h = resamp_design(L, M)
        n = L * T
        assert h.shape == (n,) and np.array_equal(h, resamp_design(L, M, T, 8.0))
        fc = 2 * 0.4 / max(L, M)
        want = fc * np.sinc(fc * (np.arange(n) - (n - 1) / 2)) * np.kaiser(n, 8.0)
        want *= L / want.sum()
        assert np.abs(h - want).max() <= 1e-12 * L, (L, M)
        assert np.array_equal(h, h[::-1]) or np.abs(h - h[::-1]).max() <= 1e-15 * L
        ripple, stop, phase = rr.design_properties(h, L, M)
        print(f"{L}/{M}: T {T}, ripple {ripple:.5f} dB, stopband {stop:.2f} dB, phase gains within {phase:.2e}")
        assert ripple <= RIPPLE_DB and stop >= STOP_DB and phase <= PHASE_GAIN, (L, M, ripple, stop, phase)
    assert np.array_equal(resamp_design(1, 1, 1), [1.0])
    for bad in [(2, 4, 8), (0, 4, 8), (513, 4, 8), (3, 4097, 8), (3, 4, 0), (3, 4, 129), (512, 1, 17)]:
        with pytest.raises(ValueError, match="resamp_design"):
            resamp_design(*bad)


# ---------------------------------------------------------------- the float32 model
def test_the_float32_model_is_inside_the_float64_gate_on_every_case(zfft_lib):
    worst = 0.0
    for i, (K, L, M, T, kind) in enumerate(rr.CASES):
        f = resamp_form(zfft_lib, K, L, M, T)
        assert f["kind"] == kind, rr.IDS[i]
        n = rr.case_len(f["span"])
        Kc = min(K, 8)                                    # (the model's columns are independent: a few stand for all)
        x = rr.noise(n, Kc, 7 + i)
        h = rr.solid_taps(L, T)
        a, ref = rr.model_push(x, 0, h, L, M), rr.ref_push(x, 0, h, L, M)
        assert a.dtype == np.float32 and a.shape == ref.shape == (rr.steps(0, n, L, M), Kc)
        err = np.abs(a.astype(np.float64) - ref)
        ratio = float((err / rr.gate(h, L, np.abs(x).max(), rr.out_indices(0, n, L, M), M)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (rr.IDS[i], ratio)
        assert err.max() > 0 or T == 1                    # (float32 it is: not the reference again)
    print(f"worst |model - ref| / gate over the cases: {worst:.4f}")


def test_the_float32_model_does_not_depend_on_the_cut_and_the_quantiser():
    K, L, M, T, n0 = 3, 5, 7, 9, 2 ** 62 - 10 ** 6
    x, h = rr.noise(300, K, 3), rr.solid_taps(L, T)
    whole = rr.model_push(x, n0, h, L, M)
    assert whole.shape == (rr.steps(n0, len(x), L, M), K)
    at, parts = 0, []
    for c in (1, 1, M - 1, T - 1, T, 50, 300 - 50 - 2 * T - M):
        lo = max(0, at - (T - 1))
        parts.append(rr.model_resamp(x[lo:at + c], n0 + lo, h, L, M, rr.out_indices(n0 + at, c, L, M)))
        at += c
    assert at == 300 and np.concatenate(parts).tobytes() == whole.tobytes()
    # rule 4: ties to even, the rails, NaN and the infinities
    y = np.float32([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 32766.5, 32767.5, -32768.5, 1e9, -1e9, np.inf, -np.inf, np.nan, 0.25])
    assert rr.quantise(y, 1.0).tolist() == [0, 2, 2, 0, -2, -2, 32766, 32767, -32768, 32767, -32768, 32767, -32768, 0, 0]
    assert rr.quantise(np.float32([1.0, -1.0, 1.0000001]), 32767.0).tolist() == [32767, -32767, 32767]
    a = np.float32([0.0, np.nan, 1.0])
    assert rr.same(a, np.float32([-0.0, np.nan, 1.0])) and not rr.same(a, np.float32([0.0, np.nan, np.nextafter(np.float32(1), 2)]))
    assert rr.same(np.int16([1, 2]), np.int16([1, 2])) and "first at (1,)" in rr.first_difference(np.int16([1, 2]), np.int16([1, 3]))


# ---------------------------------------------------------------- the chooser
def test_form_through_the_hook(zfft_lib):
    for K in (1, 2, 7, 8, 9, 64, 70, 2048):
        for L, M in [(1, 1), (3, 4), (160, 147), (64, 25), (1, 4096), (512, 1)]:
            for T in (1, 5, 16, 128):
                f = resamp_form(zfft_lib, K, L, M, T, K + 5, 1, 2 ** 40 + 3, 100003)
                if L * T > 8192:
                    assert f is None
                    continue
                assert f["kind"] == (rr.STREAMS if K >= 8 else rr.TIME), (K, L, M, T)
                table = 0 if f["kind"] == rr.STREAMS else L * f["pitch"]
                assert f["lds_bytes"] == 4 * (table + f["lanes"] * (f["halo"] + f["span"])) <= 64 * 1024
                assert f["halo"] == T - 1 and f["span"] >= 1 and f["lane_tiles"] == -(-K // f["lanes"])
                assert f["pitch"] == (0 if f["kind"] == rr.STREAMS else T | 1)
                assert f["nspans"] == -(-100003 // f["span"]) and f["ntiles"] == f["nspans"] * f["lane_tiles"]
                assert f["outputs"] == rr.steps(2 ** 40 + 3, 100003, L, M)
                assert f["p0"] == -(-(2 ** 40 + 3) * L // M) * M - (2 ** 40 + 3) * L and 0 <= f["p0"] < M
                assert f["grid"] == min(f["ntiles"], 1 << 16)
    for bad in [(0, 3, 4, 8), (2049, 3, 4, 8), (4, 0, 4, 8), (4, 513, 4, 8), (4, 3, 0, 8), (4, 3, 4097, 8), (4, 2, 4, 8),
                (4, 3, 4, 0), (4, 3, 4, 129), (4, 512, 1, 17), (4, 3, 4, 8, 3), (4, 3, 4, 8, 2 ** 31 + 1), (4, 3, 4, 8, 4, 2),
                (4, 3, 4, 8, 4, 0, 0, 0), (4, 3, 4, 8, 4, 0, 0, 2 ** 31), (4, 3, 4, 8, 4, 0, 2 ** 62 + 1, 5)]:
        assert resamp_form(zfft_lib, *bad) is None, bad


def test_resamp_form_sweep_sanitized(tmp_path):
    """The chooser, the cut, the kernel's output ranges and positions and the count over their
    domain as a stand-alone g++ program (no HIP, no Python in the child) under AddressSanitizer +
    UBSan: tests/host/resamp_form_sweep.cpp."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/host/resamp_form_sweep.cpp"
    csrc = os.path.join(ROOT, "pypanadapter_amd", "csrc")
    exe = str(tmp_path / "resamp_form_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", csrc, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "resamp_form_sweep.cpp"),
                    os.path.join(csrc, "zfft_resamp_plan.cpp"), os.path.join(csrc, "zfft_tap_plan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "resamp_form_sweep: ok" in r.stdout, r.stdout


# ---------------------------------------------------------------- names and errors
def test_new_names_signatures_and_errors_that_need_no_device(zfft_lib):
    from pypanadapter_amd import _lib
    import pypanadapter_amd as pkg
    declared = header_functions()
    for name in NAMES:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert getattr(zfft_lib, name).argtypes is not None and getattr(zfft_lib, name).restype is ctypes.c_int, name
    I32, I64, P, D = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double
    assert zfft_lib.zfft_plan_resamp.argtypes == [P, I32, I32, I32, I32, P, I32, ctypes.c_float]
    assert zfft_lib.zfft_resamp_push_device.argtypes == [P, P, I64, I64, P, P]
    assert zfft_lib.zfft_resamp_push.argtypes == [P, P, I64, I64, P, P]
    assert zfft_lib.zfft_resamp_reset.argtypes == [P, I64]
    assert zfft_lib.zfft_resamp_design.argtypes == [I32, I32, I32, D, P]
    for name in ("set_resamp", "resamp_shape", "resamp_steps", "resamp_push", "resamp_push_device", "resamp_state",
                 "resamp_reset", "resamp_info"):
        assert callable(getattr(pkg.ZoomFFT, name)), name
    assert callable(pkg.resamp_design) and isinstance(pkg.Resampler, type)
    assert callable(pkg.Resampler.for_demodulator) and callable(pkg.Resampler.for_tap)
    assert pkg.ZoomFFT.RESAMP_FORMATS == {"f32": rr.F32, "s16": rr.S16}
    # a null plan is EINVAL before anything touches a device
    v32, v64, u64, dbl = I32(), I64(), ctypes.c_uint64(), D()
    h = np.float32([1.0] * 24)
    hp = h.ctypes.data_as(P)
    r = ctypes.byref
    assert zfft_lib.zfft_plan_resamp(None, 1, 3, 4, 8, hp, 0, 1.0) == EINVAL
    assert zfft_lib.zfft_resamp_shape(None, r(v32), r(v32), r(v32), r(v32), r(v32)) == EINVAL
    assert zfft_lib.zfft_resamp_steps(None, 5, r(v64)) == EINVAL
    assert zfft_lib.zfft_resamp_push_device(None, hp, 1, 1, hp, None) == EINVAL
    assert zfft_lib.zfft_resamp_push(None, hp, 1, 1, hp, None) == EINVAL
    assert zfft_lib.zfft_resamp_state(None, r(u64)) == EINVAL
    assert zfft_lib.zfft_resamp_reset(None, 0) == EINVAL
    assert zfft_lib.zfft_resamp_info(None, r(dbl), r(dbl)) == EINVAL
    # the design's own refusals: a ratio that is not reduced, a table past 8192, a default that does not fit
    out = np.zeros(8192)
    op = out.ctypes.data_as(P)
    assert zfft_lib.zfft_resamp_design(2, 4, 8, 8.0, op) == EINVAL and b"gcd" in zfft_lib.zfft_last_error()
    assert zfft_lib.zfft_resamp_design(512, 1, 17, 8.0, op) == EINVAL and zfft_lib.zfft_resamp_design(512, 1, 16, 8.0, op) == 0
    assert rr.default_taps_per_phase(1, 16) == 256 > 128      # 1 / 16 has no default: the caller gives taps
    assert zfft_lib.zfft_resamp_design(1, 16, rr.default_taps_per_phase(1, 16), 8.0, op) == EINVAL
    with pytest.raises(ValueError, match="441 / 5000"):
        pkg.Resampler(None, 1, 500e3, 44.1e3)
    text = open(os.path.join(ROOT, "include", "zfft.h")).read()
    rule = text[text.index("/* Resampler bank:"):text.index("int zfft_plan_resamp(")]
    for clause in ("bit for bit", "last T - 1 input steps", "(T + 32) 2^-24", "ascending k", "resamp is off", "resamp_push",
                   "gcd(L, M) = 1", "ties to", "NaN gives 0", "Exactly T products", "(a_0 + a_1) + (a_2 + a_3)", "128-bit",
                   "16 ceil(max(L, M) / L)", f"ZFFT_RESAMP_F32 = {rr.F32}, ZFFT_RESAMP_S16 = {rr.S16}"):
        assert clause in rule, clause
