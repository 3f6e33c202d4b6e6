"""CPU checks of the demodulator bank's host side: the reference itself against closed forms (an FM
tone, an AM envelope, an SSB tone, the power of a constant) and its own invariance under cutting;
the design against scipy; the output counts against the rule's formula (around 2^32 and 2^40
too); the form chooser through its hook over a grid and, over its whole domain, as a stand-alone
program under ASan + UBSan (tests/host/demod_form_sweep.cpp); the FM signals' seeds against the
0.9 pi condition; the C-ABI's new names, their ctypes signatures and the errors that need no
device."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.signal

import demod_ref as dr
from test_host import header_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["zfft_plan_demod", "zfft_demod_shape", "zfft_demod_mode", "zfft_demod_steps", "zfft_demod_push_device",
         "zfft_demod_push", "zfft_demod_state", "zfft_demod_reset", "zfft_demod_info", "zfft_demod_design"]
EINVAL = -1
FORM = ("kind", "lanes", "outs", "span", "halo", "lds_bytes", "stream_tiles", "nspans", "ntiles", "outputs", "r0", "grid")
TIME, STREAMS = 0, 1


def demod_form(lib, K, Ta, Da, step_stride, stream_stride, n0=0, steps=1):
    """The form dict of zfft__demod_form (the shape's form and the cut of a push), or None where it
    refuses."""
    hook = lib.zfft__demod_form
    hook.argtypes = [ctypes.c_int32] * 3 + [ctypes.c_int64] * 2 + [ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p]
    hook.restype = ctypes.c_int
    form = np.zeros(len(FORM), np.int64)
    if hook(K, Ta, Da, step_stride, stream_stride, n0, steps, form.ctypes.data_as(ctypes.c_void_p)):
        return None
    return dict(zip(FORM, map(int, form)))


# ---------------------------------------------------------------- the reference against closed forms
def test_reference_fm_tone_is_twice_its_offset():
    n, f = 400, 0.0625                                   # cycles per step: exact in binary
    x = np.exp(2j * np.pi * f * np.arange(n))[:, None]
    d = dr.detect(x, 0, dr.FM, 0)
    assert d[0, 0] == 0.0                                # the product with the zero before the start
    assert np.abs(d[1:, 0] - 2 * f).max() <= 1e-13       # +-1 is +-half the rate
    d = dr.detect(np.conj(x), 5, dr.FM, 0)
    assert np.abs(d[1:, 0] + 2 * f).max() <= 1e-13
    # through a unit-gain filter the tone stays 2 f once the window is full
    g = np.full(8, 0.125)
    a = dr.ref_push(x, 0, dr.FM, 0, g, 4)
    assert np.abs(a[3:, 0] - 2 * f).max() <= 1e-13 and a.shape == (100, 1)


def test_reference_am_envelope_ssb_tone_and_power():
    n = 512
    t = np.arange(n)
    env = 1 + 0.5 * np.cos(2 * np.pi * 0.01 * t)
    x = (env * np.exp(2j * np.pi * 0.2 * t + 0.3j))[:, None]
    assert np.abs(dr.detect(x, 0, dr.AM, 0)[:, 0] - env).max() <= 1e-13
    assert np.abs(dr.detect(x, 0, dr.POWER, 0)[:, 0] - env ** 2).max() <= 1e-13
    c = np.full((n, 1), 0.6 - 0.8j)
    assert np.abs(dr.detect(c, 7, dr.POWER, 0)[:, 0] - 1.0).max() <= 1e-15
    # SSB: a tone at +f with a BFO word w gives a real tone at f + w / 2^32, whatever the count
    # (the tone's frequency is a word too, so that every phase is an exact integer mod 2^32)
    fw, w = 2 ** 27, 3 * 2 ** 26 + 12345
    turns = lambda word, n0: np.array([(word * (n0 + i)) % 2 ** 32 for i in range(n)], dtype=np.float64) / 2 ** 32
    for n0 in (0, 2 ** 32 - 100, 2 ** 40 + 3):
        x = np.exp(2j * np.pi * turns(fw, n0))[:, None]
        got = dr.detect(x, n0, dr.SSB, w)[:, 0]
        assert np.abs(got - np.cos(2 * np.pi * turns(fw + w, n0))).max() <= 1e-12, n0
        lsb = dr.detect(x, n0, dr.SSB, -w)[:, 0]          # a negative word: the difference frequency
        assert np.abs(lsb - np.cos(2 * np.pi * turns(fw - w, n0))).max() <= 1e-12, n0


def test_reference_does_not_depend_on_the_cut_and_mixes_modes():
    K, Ta, Da, n0 = 4, 9, 3, 2 ** 32 - 50
    x = dr.noise_and_tones(300, K, 3)
    g = dr.audio_taps(Ta, Da)
    modes, words = [dr.AM, dr.FM, dr.SSB, dr.POWER], [0, 0, -12345678, 0]
    ms = dr.step_indices(n0, len(x), Da)
    whole = dr.ref_demod(x, n0, modes, words, g, Da, ms)
    assert whole.shape == (dr.steps(n0, len(x), Da), K)
    late = [m for m in ms if m * Da >= n0 + 120]
    a = late[0] * Da - n0 - Ta                            # Ta inputs before the first output: the carry
    part = dr.ref_demod(x[a:], n0 + a, modes, words, g, Da, late)
    assert np.abs(part - whole[len(ms) - len(late):]).max() <= 1e-12
    for s, (m, w) in enumerate(zip(modes, words)):        # a stream alone is its column
        one = dr.ref_demod(x[:, s:s + 1], n0, m, w, g, Da, ms)
        assert np.array_equal(one[:, 0], whole[:, s])


def test_the_fm_signals_stay_inside_the_branch(zfft_lib):
    """The signals the GPU tests draw (every case at the length its form asks for, and the fixed
    ones): every |arg z| <= 0.9 pi on the float64 reference."""
    drawn = {}
    for i, (K, Ta, Da, layout) in enumerate(dr.CASES):
        f = demod_form(zfft_lib, K, Ta, Da, *dr.strides(layout, K, 5000))
        drawn[dr.fm_seed(i)] = (dr.case_len(f["span"]), K)
    drawn.update({31: (4096, 64), 32: (3000, 64), 35: (1500, 64), 36: (2000, 8), 37: (3000, 16)})
    for seed, (n, K) in drawn.items():
        x = dr.fm_signal(n, K, seed)
        assert dr.fm_arg_ok(x), seed
        assert 0.94 <= np.abs(x).min() and np.abs(x).max() <= 1.06
        d = dr.detect(x, 0, dr.FM, 0)
        assert 0.5 < np.abs(d).max() <= dr.FM_ARG_MAX


# ---------------------------------------------------------------- the library's pure pieces
def test_design_is_scipys_firwin(zfft_lib):
    from pypanadapter_amd.engine import demod_design, tap_design
    for T, cutoff, beta in [(1, 0.4, 8.0), (9, 0.4, 8.0), (33, 0.1, 8.0), (513, 0.4 / 64, 8.0), (1024, 0.01, 5.0)]:
        h = demod_design(T, cutoff, beta)
        want = scipy.signal.firwin(T, 2 * cutoff, window=("kaiser", beta))
        assert h.dtype == np.float64 and np.abs(h - want).max() <= 1e-12, (T, cutoff, beta)
        assert np.array_equal(h, tap_design(T, cutoff, beta))
    for bad in [(0, 0.1, 8.0), (1025, 0.1, 8.0), (5, 0.0, 8.0), (5, 0.5, 8.0), (5, 0.1, -1.0)]:
        with pytest.raises(ValueError):
            demod_design(*bad)
    assert zfft_lib.zfft_demod_design(5, 0.1, 8.0, None) == EINVAL


def test_output_counts_are_the_rule(zfft_lib):
    hook = zfft_lib.zfft__demod_steps
    hook.argtypes, hook.restype = [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int32], ctypes.c_int64
    for n0 in (0, 1, 63, 64, 2 ** 32 - 100, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 3, 2 ** 62 - 2 ** 31):
        for Da in (1, 2, 3, 4, 8, 63, 64):
            for n in (0, 1, 2, Da - 1, Da, Da + 1, 1023, 5000, 2 ** 31 - 1):
                assert hook(n0, n, Da) == dr.steps(n0, n, Da) == len(range(dr.ceil_div(n0, Da), dr.ceil_div(n0 + n, Da)))
    # cutting a stretch never changes the total
    for n0, Da in ((0, 4), (2 ** 32 - 100, 64), (2 ** 40 + 3, 3)):
        cuts = [1, 1, 7, Da - 1 or 1, 64, 63, 1023, 4000]
        at, total = n0, 0
        for n in cuts:
            total += hook(at, n, Da)
            at += n
        assert total == hook(n0, sum(cuts), Da) == dr.steps(n0, sum(cuts), Da)
    assert hook(0, -1, 4) == 0 and hook(0, 5, 0) == 0


def test_form_chooser_through_the_hook(zfft_lib):
    for K in (1, 3, 5, 7, 8, 9, 16, 64, 65, 1024):
        for Ta in (1, 8, 17, 33, 65, 256, 1024):
            for Da in (1, 2, 3, 8, 64):
                for ss, ts in ((K, 1), (1, 5000), (1, 1 if K > 1 else 0), (2 * K, 1), (5, 3)):
                    for n0, n in ((0, 1), (5, 4999), (2 ** 32 - 100, 30001), (2 ** 40 + 3, 2 ** 31 - 1)):
                        f = demod_form(zfft_lib, K, Ta, Da, ss, ts, n0, n)
                        assert f is not None, (K, Ta, Da, ss, ts)
                        streams = ts == 1 and K >= 8
                        assert f["kind"] == (STREAMS if streams else TIME)
                        L = f["lanes"]
                        assert (8 <= L <= 64 and L & (L - 1) == 0 and L < 2 * K) if streams else L == 1
                        assert f["stream_tiles"] == -(-K // L)
                        assert f["halo"] == Ta - 1 and f["span"] == f["outs"] * Da >= Da
                        last = f["halo"] + f["span"] - 1
                        rows = last + (last >> 5) + 1 if f["kind"] == TIME else last + 1
                        assert f["lds_bytes"] == 4 * L * rows <= 64 * 1024 < 160 * 1024
                        assert f["nspans"] == -(-n // f["span"]) and f["ntiles"] == f["nspans"] * f["stream_tiles"]
                        assert f["grid"] == min(f["ntiles"], 1 << 16)
                        assert 0 <= f["r0"] < Da and (n0 + f["r0"]) % Da == 0
                        assert f["outputs"] == dr.steps(n0, n, Da)
    # the cases the GPU tests name
    assert demod_form(zfft_lib, 64, 65, 8, 64, 1)["lanes"] == 64
    assert demod_form(zfft_lib, 1024, 17, 2, 1024, 1)["stream_tiles"] == 16
    assert demod_form(zfft_lib, 16, 256, 64, 16, 1)["lanes"] == 16
    assert demod_form(zfft_lib, 3, 8, 3, 3, 1)["kind"] == TIME          # a row of 3 streams is 24 bytes
    assert demod_form(zfft_lib, 64, 33, 4, 1, 77777)["kind"] == TIME    # far apart
    for bad in [(0, 8, 2, 1, 1), (1025, 8, 2, 1025, 1), (4, 0, 2, 4, 1), (4, 1025, 2, 4, 1), (4, 8, 0, 4, 1), (4, 8, 65, 4, 1),
                (4, 8, 2, 0, 1), (4, 8, 2, 4, 0), (4, 8, 2, 2 ** 31 + 1, 1), (4, 8, 2, 4, 1, 0, 0), (4, 8, 2, 4, 1, 0, 2 ** 31),
                (4, 8, 2, 4, 1, 2 ** 62 + 1, 5)]:
        assert demod_form(zfft_lib, *bad) is None, bad


def test_demod_form_sweep_sanitized(tmp_path):
    """The chooser, the cut, the kernel's output ranges and the counts over their domain as a
    stand-alone g++ program (no HIP, no Python in the child) under AddressSanitizer + UBSan:
    tests/host/demod_form_sweep.cpp."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/host/demod_form_sweep.cpp"
    csrc = os.path.join(ROOT, "pypanadapter_amd", "csrc")
    exe = str(tmp_path / "demod_form_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", csrc, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "demod_form_sweep.cpp"),
                    os.path.join(csrc, "zfft_demod_plan.cpp"), os.path.join(csrc, "zfft_tap_plan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "demod_form_sweep: ok" in r.stdout, r.stdout


def test_new_names_signatures_and_null_plan_errors(zfft_lib):
    from pypanadapter_amd import _lib
    import pypanadapter_amd as pkg
    declared = header_functions()
    for name in NAMES:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert getattr(zfft_lib, name).argtypes is not None and getattr(zfft_lib, name).restype is ctypes.c_int, name
    I32, I64, P = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    assert zfft_lib.zfft_plan_demod.argtypes == [P, I32, I32, I32, P]
    assert zfft_lib.zfft_demod_mode.argtypes == [P, I32, I32, I32, I64]
    assert zfft_lib.zfft_demod_push_device.argtypes == [P, P, I64, I64, I64, P, P]
    assert zfft_lib.zfft_demod_push.argtypes == [P, P, I64, I64, I64, P, P]
    assert zfft_lib.zfft_demod_reset.argtypes == [P, I64]
    assert zfft_lib.zfft_demod_design.argtypes == [I32, ctypes.c_double, ctypes.c_double, P]
    for name in ("set_demod", "demod_mode", "demod_push", "demod_push_device", "demod_steps", "demod_reset", "demod_info",
                 "demod_shape", "demod_state"):
        assert callable(getattr(pkg.ZoomFFT, name)), name
    assert callable(pkg.demod_design) and isinstance(pkg.Demodulator, type)
    assert callable(pkg.Demodulator.for_channelizer) and callable(pkg.Demodulator.for_tap)
    assert pkg.ZoomFFT.DEMOD_MODES == dr.MODES
    # a null plan is EINVAL before anything touches a device
    v32, v64, u64, dbl = I32(), I64(), ctypes.c_uint64(), ctypes.c_double()
    h = np.float32([1.0] * 8)
    hp = h.ctypes.data_as(P)
    r = ctypes.byref
    assert zfft_lib.zfft_plan_demod(None, 1, 8, 1, hp) == EINVAL
    assert zfft_lib.zfft_demod_shape(None, r(v32), r(v32), r(v32)) == EINVAL
    assert zfft_lib.zfft_demod_mode(None, 0, 1, 0, 0) == EINVAL
    assert zfft_lib.zfft_demod_steps(None, 5, r(v64)) == EINVAL
    assert zfft_lib.zfft_demod_push_device(None, hp, 1, 1, 1, hp, None) == EINVAL
    assert zfft_lib.zfft_demod_push(None, hp, 1, 1, 1, hp, None) == EINVAL
    assert zfft_lib.zfft_demod_state(None, r(u64)) == EINVAL
    assert zfft_lib.zfft_demod_reset(None, 0) == EINVAL
    assert zfft_lib.zfft_demod_info(None, r(dbl), r(dbl)) == EINVAL
    text = open(os.path.join(ROOT, "include", "zfft.h")).read()
    rule = text[text.index("/* Demodulator bank:"):text.index("int zfft_plan_demod(")]
    for clause in ("bit for bit", "last Ta complex inputs", "(Ta + 32) 2^-24", "ascending k", "demod is off", "demod_push",
                   "0.9 pi", "ZFFT_DEMOD_EPS_FM", "band-pass", "mod 2^32", "(a_0 + a_1) + (a_2 + a_3)"):
        assert clause in rule, clause
    # the header's constants are the reference's
    for name, v in (("AM", dr.AM), ("FM", dr.FM), ("SSB", dr.SSB), ("POWER", dr.POWER)):
        assert f"ZFFT_DEMOD_{name} = {v}" in rule
    assert f"#define ZFFT_DEMOD_EPS_FM {dr.EPS_FM}\n" in rule and dr.EPS_FM <= 16


# ---------------------------------------------------------------- the rule in float32 (demod_ref's model)
def test_the_float32_model_is_inside_the_float64_gate_on_every_case(zfft_lib):
    """detect_f32 and fir_f32 (the header's rules 2 and 3, rounded where the header rounds) against
    the float64 reference under rule 6's gate, on the GPU tests' cases and signals, in every mode the
    host models: AM, POWER and SSB at the four quarter-turn words."""
    for i, (K, Ta, Da, layout) in enumerate(dr.CASES):
        f = demod_form(zfft_lib, K, Ta, Da, *dr.strides(layout, K, 5000))
        n = dr.case_len(f["span"])
        x = dr.noise_and_tones(n, K, 7 + i)
        g = dr.audio_taps(Ta, Da)
        xmax = np.abs(x).max()
        for m, words in ((dr.AM, 0), (dr.POWER, 0), (dr.SSB, np.array(dr.QUARTER_WORDS)[np.arange(K) % 4])):
            a = dr.model_push(x, 0, m, words, g, Da)
            ref = dr.ref_push(x, 0, m, words, g, Da)
            assert a.dtype == np.float32 and a.shape == ref.shape == (dr.steps(0, n, Da), K)
            ratio = np.abs(a.astype(np.float64) - ref).max() / dr.gate(g, m, xmax)
            assert ratio <= 1.0, (dr.IDS[i], m, ratio)
            assert np.abs(a.astype(np.float64) - ref).max() > 0 or Ta == 1    # (float32 it is: not the reference again)
    # FM's z and its zero predicate: the float64 product within two roundings, zero where x or p is
    x = dr.fm_signal(500, 3, 5)
    x[[7, 100, 101]] = 0
    z_re, z_im = dr.fm_z_f32(x)
    z = x.astype(np.complex128) * np.conj(np.vstack([np.zeros((1, 3)), x[:-1].astype(np.complex128)]))
    assert np.abs(z_re - z.real).max() <= 3 * dr.U * 1.2 and np.abs(z_im - z.imag).max() <= 3 * dr.U * 1.2
    assert np.array_equal(dr.fm_zero_f32(x), z == 0) and dr.fm_zero_f32(x).sum() == 3 * 6   # steps 0, 7, 8, 100, 101, 102
    tiny = np.full((4, 1), 2.0 ** -75 * (1 + 1j), np.complex64)         # x != 0 but both products underflow
    assert dr.fm_zero_f32(tiny).all() and not (tiny == 0).any()


def test_the_float32_model_does_not_depend_on_the_cut():
    K, Ta, Da, n0 = 4, 9, 3, 2 ** 32 - 50
    x = dr.noise_and_tones(300, K, 3)
    g = dr.audio_taps(Ta, Da)
    modes, words = [dr.AM, dr.SSB, dr.SSB, dr.POWER], [0, 2 ** 30, -2 ** 31, 0]
    whole = dr.model_push(x, n0, modes, words, g, Da)
    assert whole.shape == (dr.steps(n0, len(x), Da), K)
    at, parts = 0, []
    for c in (1, 1, Da - 1, Ta - 1, Ta, 50, 300 - 50 - 2 * Ta - Da):
        lo = max(0, at - (Ta - 1))                        # the carry: Ta - 1 detected steps before the cut
        d = dr.detect_f32(x[lo:at + c], n0 + lo, modes, words)
        parts.append(dr.fir_f32(d, g, Da, n0 + at, c, first=n0 + lo))
        at += c
    assert at == 300 and np.concatenate(parts).tobytes() == whole.tobytes()
    for s in range(K):                                    # a stream alone is its column
        assert dr.model_push(x[:, s:s + 1], n0, modes[s], words[s], g, Da).tobytes() == whole[:, s:s + 1].tobytes()
    # the comparison the exact tests use: NaN equals NaN, +0 equals -0, nothing else is forgiven
    a = np.float32([0.0, np.nan, 1.0])
    assert dr.same(a, np.float32([-0.0, np.nan, 1.0])) and not dr.same(a, np.float32([0.0, np.nan, np.nextafter(np.float32(1), 2)]))
    assert not dr.same(a, a.astype(np.float64)) and "first at (2,)" in dr.first_difference(a, np.float32([0, np.nan, 2]))
