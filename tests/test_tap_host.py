"""CPU checks of the channel taps' host side: the Kaiser design against scipy, the modulated table
against float64, the output counts against the rule's formula (around 2^32 and 2^40 too), the
form chooser through its hook and, over its whole domain, as a stand-alone program under ASan +
UBSan (tests/host/tap_form_sweep.cpp); the C-ABI's new names, their ctypes signatures and the
errors that need no device; and the reference's own invariance under cutting."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.signal

import tap_ref as tp
from test_host import header_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["zfft_plan_taps", "zfft_tap_shape", "zfft_tap_open", "zfft_tap_close", "zfft_tap_info", "zfft_tap_counts",
         "zfft_tap_push_device", "zfft_tap_push", "zfft_tap_state", "zfft_tap_reset", "zfft_tap_design",
         "zfft_tap_table"]
EINVAL = -1


def test_design_is_scipys_firwin(zfft_lib):
    from pypanadapter_amd.engine import tap_design
    for T, cutoff, beta in [(1, 0.4, 8.0), (2, 0.2, 8.0), (3, 0.1, 5.0), (25, 0.4 / 3, 8.0), (65, 0.05, 8.0),
                            (64, 0.05, 0.0), (257, 0.4 / 32, 8.0), (1601, 0.002, 8.0), (2048, 0.4 / 512, 14.0)]:
        h = tap_design(T, cutoff, beta)
        want = scipy.signal.firwin(T, 2 * cutoff, window=("kaiser", beta))
        assert h.dtype == np.float64 and np.abs(h - want).max() <= 1e-12, (T, cutoff, beta)
        assert abs(h.sum() - 1.0) <= 1e-12
    for bad in [(0, 0.1, 8.0), (2049, 0.1, 8.0), (5, 0.0, 8.0), (5, 0.5, 8.0), (5, -0.1, 8.0), (5, np.nan, 8.0),
                (5, 0.1, -1.0), (5, 0.1, np.inf)]:
        with pytest.raises(ValueError):
            tap_design(*bad)
    assert zfft_lib.zfft_tap_design(5, 0.1, 8.0, None) == EINVAL


def test_table_is_the_rule_within_one_rounding(zfft_lib):
    from pypanadapter_amd.engine import tap_table
    rng = np.random.default_rng(3)
    for T, fw in [(1, 0), (1, 12345), (65, 1), (65, -1), (257, -2 ** 31), (1601, 2 ** 31 - 1), (2048, 0x1234567)]:
        h = tp.solid_taps(T, T) if T > 1 else np.float32([0.75])
        if T == 257:
            h = (h * rng.uniform(1e-6, 1.0, T)).astype(np.float32)
        c = tap_table(fw, h)
        ph = [((fw % tp.TWO32) * k) % tp.TWO32 for k in range(T)]          # exact integers
        want = h.astype(np.float64) * np.exp(2j * np.pi * np.array(ph, dtype=np.float64) / tp.TWO32)
        for got, ref in ((c.real, want.real), (c.imag, want.imag)):
            # one float32 rounding of the float64 value (whose own error is 1e-16 relative to |h|)
            assert np.all(np.abs(got.astype(np.float64) - ref) <= 2.0 ** -24 * np.abs(ref) + 1e-15 * np.abs(h)), (T, fw)
        if fw == 0:
            assert np.array_equal(c.real, h) and not c.imag.any()
    h1 = np.float32([1.0])
    out = np.zeros(2, np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert zfft_lib.zfft_tap_table(0, 0, p(h1), p(out)) == EINVAL
    assert zfft_lib.zfft_tap_table(0, 2049, p(h1), p(out)) == EINVAL
    assert zfft_lib.zfft_tap_table(2 ** 31, 1, p(h1), p(out)) == EINVAL
    assert zfft_lib.zfft_tap_table(-2 ** 31 - 1, 1, p(h1), p(out)) == EINVAL
    assert zfft_lib.zfft_tap_table(0, 1, None, p(out)) == EINVAL and zfft_lib.zfft_tap_table(0, 1, p(h1), None) == EINVAL
    assert b"tap_table" in zfft_lib.zfft_last_error()


def _count_hook(lib):
    hook = lib.zfft__tap_count
    hook.argtypes, hook.restype = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int32], ctypes.c_int64
    return hook


def test_counts_are_the_formula(zfft_lib):
    hook = _count_hook(zfft_lib)
    n0s = [0, 1, 7, 199, 200, 201, 4096, 2 ** 32 - 100, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 3, 2 ** 62 - 2 ** 31]
    for n0 in n0s:
        for D in (1, 2, 3, 8, 32, 200, 511, 512):
            for n in (0, 1, 2, D - 1, D, D + 1, 1023, 5000, 2 ** 31 - 1):
                for n_open in {0, n0 // 2, max(0, n0 - D), max(0, n0 - 1), n0, n0 + 1, n0 + n // 2, n0 + n, n0 + n + 5}:
                    assert hook(n0, n_open, n, D) == tp.count(n0, n_open, n, D), (n0, n_open, n, D)
    # cutting a stretch never changes the total
    for n0, D in ((2 ** 32 - 100, 200), (2 ** 40 + 3, 3), (5, 8)):
        cuts = [1, 1, 7, D - 1, 64, 63, 1023, 4000]
        at, total = n0, 0
        for n in cuts:
            total += hook(at, n0, n, D)
            at += n
        assert total == hook(n0, n0, sum(cuts), D) == tp.count(n0, n0, sum(cuts), D)


def tap_form(lib, n0, n, max_len, taps):
    """(form dict, items) of zfft__tap_form for taps = [(fw, D, T, n_open)], or None where it refuses."""
    hook = lib.zfft__tap_form
    P = ctypes.c_void_p
    hook.argtypes = [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, P, P, P, P, P, P]
    hook.restype = ctypes.c_int
    k = len(taps)
    fw = np.array([t[0] for t in taps], dtype=np.int64)
    D = np.array([t[1] for t in taps], dtype=np.int32)
    T = np.array([t[2] for t in taps], dtype=np.int32)
    no = np.array([t[3] for t in taps], dtype=np.uint64)
    form, items = np.zeros(8, np.int64), np.zeros((max(k, 1), 6), np.int64)
    p = lambda a: a.ctypes.data_as(P)
    if hook(n0, n, max_len, k, p(fw), p(D), p(T), p(no), p(form), p(items)):
        return None
    names = ("span", "halo", "lds_bytes", "first_span", "grid", "ntaps", "total", "pad_shift")
    return dict(zip(names, map(int, form))), items[:k]


def test_form_chooser_through_the_hook(zfft_lib):
    taps = [(tp.freq_word(0.1, 1.0), 8, 65, 0), (-5, 200, 1601, 0), (2 ** 31 - 1, 1, 1, 0), (7, 512, 2048, 0)]
    for n0 in (0, 4093, 2 ** 32 - 100, 2 ** 40 + 3):
        for n in (1, 511, 512, 513, 1300, 524288, 524289, 4096 * 1024 + 77, 4096 * 299008, 2 ** 31 - 1):
            opened = [(fw, D, T, n0 if i % 2 else n0 // 3) for i, (fw, D, T, _) in enumerate(taps)]
            f, items = tap_form(zfft_lib, n0, n, 2048, opened)
            S = f["span"]
            assert S in (512, 1024, 2048, 4096) and f["halo"] == 2047 and f["ntaps"] == 4
            last, sh = f["halo"] + S - 1, f["pad_shift"]
            assert sh in (31, 3, 4, 5, 6, 7, 8, 9) and f["lds_bytes"] == 8 * (last + (last >> sh) + 1) <= 64 * 1024
            spans = -(-n // S)
            assert f["first_span"] == 0 and f["grid"] == spans             # every sample in exactly one span
            assert (S == 512 or spans >= 1024) and (S == 4096 or -(-n // (2 * S)) < 1024)
            counts = [tp.count(n0, no, n, D) for _, D, _, no in opened]
            assert items[:, 4].tolist() == counts and f["total"] == sum(counts)
            assert items[:, 1].tolist() == [0] + np.cumsum(counts)[:-1].tolist()   # offsets: the prefix sums
            for (fw, D, T, no), it in zip(opened, items):
                r0 = int(it[0])
                assert 0 <= r0 < D and (n0 + r0) % D == 0
                assert int(it[2]) == ((fw % tp.TWO32) * (n0 + r0)) % tp.TWO32    # rot's phase word, exact
                assert int(it[3]) == ((fw % tp.TWO32) * D) % tp.TWO32
            # no tap open: only the spans that hold the next carry
            g, _ = tap_form(zfft_lib, n0, n, 2048, [])
            assert g["ntaps"] == 0 and g["total"] == 0 and g["halo"] == 0
            assert g["first_span"] * g["span"] <= max(0, n - 2047) < (g["first_span"] + 1) * g["span"]
            assert g["first_span"] + g["grid"] == -(-n // g["span"])
    ok = [(0, 8, 65, 0)]
    assert tap_form(zfft_lib, 0, 100, 65, ok) is not None
    for bad in [(0, 0, 65, ok), (0, 2 ** 31, 65, ok), (0, 100, 64, ok), (0, 100, 2049, ok), (2 ** 62 + 1, 100, 65, ok),
                (0, 100, 65, [(0, 0, 65, 0)]), (0, 100, 65, [(0, 513, 65, 0)]), (0, 100, 65, [(0, 8, 0, 0)]),
                (0, 100, 65, [(2 ** 31, 8, 65, 0)]), (0, 100, 65, [(0, 8, 65, 1)])]:
        assert tap_form(zfft_lib, *bad) is None, bad


def test_tap_form_sweep_sanitized(tmp_path):
    """The chooser, the counts and the table code over their domain as a stand-alone g++ program (no
    HIP, no Python in the child) under AddressSanitizer + UBSan: tests/host/tap_form_sweep.cpp."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/host/tap_form_sweep.cpp"
    csrc = os.path.join(ROOT, "pypanadapter_amd", "csrc")
    exe = str(tmp_path / "tap_form_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", csrc, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "tap_form_sweep.cpp"),
                    os.path.join(csrc, "zfft_tap_plan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tap_form_sweep: ok" in r.stdout, r.stdout


def test_new_names_signatures_and_null_plan_errors(zfft_lib):
    from pypanadapter_amd import _lib
    declared = header_functions()
    for name in NAMES:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert getattr(zfft_lib, name).argtypes is not None and getattr(zfft_lib, name).restype is ctypes.c_int, name
    I32, I64, P = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    assert zfft_lib.zfft_tap_open.argtypes == [P, I32, I64, I32, I32, P]
    assert zfft_lib.zfft_tap_push_device.argtypes == [P, P, I64, P, P]
    assert zfft_lib.zfft_tap_push.argtypes == [P, P, I64, P, P]
    assert zfft_lib.zfft_tap_reset.argtypes == [P, I64] and zfft_lib.zfft_tap_counts.argtypes == [P, I64, P]
    assert zfft_lib.zfft_tap_design.argtypes == [I32, ctypes.c_double, ctypes.c_double, P]
    assert zfft_lib.zfft_tap_table.argtypes == [I64, I32, P, P]
    # a null plan is EINVAL before anything touches a device
    v32, v64, u64, dbl = I32(), I64(), ctypes.c_uint64(), ctypes.c_double()
    h = np.float32([1.0])
    hp = h.ctypes.data_as(P)
    r = ctypes.byref
    assert zfft_lib.zfft_plan_taps(None, 4, 65) == EINVAL
    assert zfft_lib.zfft_tap_shape(None, r(v32), r(v32)) == EINVAL
    assert zfft_lib.zfft_tap_open(None, 0, 0, 1, 1, hp) == EINVAL
    assert zfft_lib.zfft_tap_close(None, 0) == EINVAL
    assert zfft_lib.zfft_tap_info(None, 0, r(v32), r(v64), r(v32), r(v32), r(u64), r(dbl)) == EINVAL
    assert zfft_lib.zfft_tap_counts(None, 5, hp) == EINVAL
    assert zfft_lib.zfft_tap_push_device(None, hp, 1, hp, None) == EINVAL
    assert zfft_lib.zfft_tap_push(None, hp, 1, hp, None) == EINVAL
    assert zfft_lib.zfft_tap_state(None, r(u64)) == EINVAL
    assert zfft_lib.zfft_tap_reset(None, 0) == EINVAL
    text = open(os.path.join(ROOT, "include", "zfft.h")).read()
    rule = text[text.index("/* Channel taps:"):text.index("int zfft_plan_taps(")]
    for clause in ("mod 2^32", "bit for bit", "max_len - 1", "(T + 32) 2^-24", "ascending k", "ZFFT_EUNSUPPORTED"):
        assert clause in rule, clause


def test_the_reference_does_not_depend_on_the_cut(zfft_lib):
    """ref_tap over a whole stream equals ref_tap over any window of it that holds the T - 1 samples
    before the outputs asked for -- the property the device carry has to keep; and the outputs the
    reference cuts that way are as many as the library counts for the same cut (zfft__tap_count)."""
    hook = _count_hook(zfft_lib)
    x = tp.noise_and_tones(3000, 5).astype(np.complex128)
    for D, T in tp.DT_TAPS:
        h = tp.solid_taps(T, 10 + D)
        fw = tp.freq_word(0.0731, 1.0)
        n0 = 2 ** 32 - 700
        ms = tp.outputs(n0, n0, x.size, D)
        whole = tp.ref_tap(x, n0, fw, D, h, ms)
        late = ms[ms * D >= n0 + 1700]
        a = int(late[0]) * D - n0 - (T - 1)
        assert a >= 0
        part = tp.ref_tap(x[a:], n0 + a, fw, D, h, late)
        assert np.array_equal(part, whole[ms.size - late.size:])
        assert whole.size == tp.count(n0, n0, x.size, D) == hook(n0, n0, x.size, D)
        # the library's counts for the two pushes [n0, n0 + 1700) and the rest: the reference's cut
        assert hook(n0 + 1700, n0, x.size - 1700, D) == late.size
        assert hook(n0, n0, 1700, D) == ms.size - late.size


# ---------------------------------------------------------------- the rule in float32 (tap_ref's model)
def _f32_cases(D, T):
    """(fw, h) of the exact comparisons: fw = 0 and a quarter-turn word with a fully complex table
    (or, where D leaves none, 2^30 and -2^31), with solid taps and with the default design."""
    from pypanadapter_amd.engine import tap_design
    q = tp.quarter_word(D)
    words = [0, q] if q is not None else [0, 2 ** 30, -2 ** 31]
    return [(fw, h) for fw in words for h in (tp.solid_taps(T, 100 + D), tap_design(T, 0.4 / D, 8.0).astype(np.float32))]


def test_the_float32_model_is_inside_the_float64_gate_and_does_not_depend_on_the_cut(zfft_lib):
    """tap_f32 (the header's rule 7, rounded where the header rounds, on zfft_tap_table's c[k])
    against the float64 reference under the gate on the GPU tests' push; and equal to itself over a
    window that holds the T - 1 samples before the outputs asked for."""
    from pypanadapter_amd.engine import tap_table
    for D, T in tp.DT_TAPS:
        n = 2 * 512 + 301 + (T if T > 1024 else 0)
        x = tp.noise_and_tones(n, 7 + D)
        for fw, h in _f32_cases(D, T):
            assert (fw * D) % 2 ** 30 == 0 and -2 ** 31 <= fw < 2 ** 31
            c = tap_table(fw, h)
            if fw % 2 ** 30:
                assert T < 3 or (np.abs(c.real[1:]).min() > 0 and np.abs(c.imag[1:3]).min() > 0)   # fully complex
            n0 = 2 ** 32 - 100 if D == 8 else 0
            y = tp.model_push(x, n0, fw, D, c)
            ref = tp.ref_push(x, n0, fw, D, h)
            assert y.dtype == np.complex64 and y.shape == ref.shape
            err = np.abs(y.astype(np.complex128) - ref).max()
            assert err <= tp.gate(h, np.abs(x).max()), (D, T, fw, err)
            ms = tp.outputs(n0, n0, n, D)
            late = ms[ms * D >= n0 + 700]
            a = int(late[0]) * D - n0 - (T - 1)
            if a >= 0:
                assert tp.tap_f32(x[a:], n0 + a, fw, D, c, late).tobytes() == y[ms.size - late.size:].tobytes()
    assert tp.quarter_word(32) == 5 * 2 ** 25 and tp.quarter_word(3) is None and tp.quarter_word(200) == 5 * 2 ** 27
