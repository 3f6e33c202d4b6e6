"""CPU checks of the row history: the declared and exported names; the quantiser of include/zfft.h
(zfft_history_codes / _values) against history_ref bit for bit, with the rule's three properties
-- idempotent over every code, monotone, within 0.513 step inside the range -- checked on the
CPU reference itself; and the pure form chooser (zfft_history_plan.h) swept through its hook and
as a stand-alone sanitised program.  No call reaches a GPU here."""
import ctypes
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import history_ref as hr
from test_host import header_functions

NAMES = ["zfft_plan_history", "zfft_history_shape", "zfft_history_push_device", "zfft_history_push",
         "zfft_history_state", "zfft_history_read_device", "zfft_history_read", "zfft_history_view_device",
         "zfft_history_view", "zfft_history_render", "zfft_history_replay_viewport", "zfft_history_reset",
         "zfft_history_codes", "zfft_history_values"]
EINVAL = -1


def test_new_names_are_declared_and_exported(zfft_lib):
    from pypanadapter_amd import _lib
    declared = header_functions()
    for name in NAMES:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert getattr(zfft_lib, name).argtypes is not None, name
    assert _lib.HISTORY_FORMATS == {"f32": 0, "u16": 1, "u8": 2} == hr.FORMATS
    assert ctypes.sizeof(_lib.zfft_history_window) == 32
    text = open(os.path.join(ROOT, "include", "zfft.h")).read()
    assert "ZFFT_HISTORY_F32 = 0, ZFFT_HISTORY_U16 = 1, ZFFT_HISTORY_U8 = 2" in text


def lib_codes(lib, fmt, lo, hi, v):
    v = np.ascontiguousarray(v, dtype=np.float32)
    out = np.empty(v.size, np.uint16)
    assert lib.zfft_history_codes(hr.FORMATS[fmt], lo, hi, v.ctypes.data, v.size, out.ctypes.data) == 0
    return out


def lib_values(lib, fmt, lo, hi, codes):
    codes = np.ascontiguousarray(codes, dtype=np.uint16)
    out = np.empty(codes.size, np.float32)
    assert lib.zfft_history_values(hr.FORMATS[fmt], lo, hi, codes.ctypes.data, codes.size, out.ctypes.data) == 0
    return out


def same_bits(a, b, what):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=str(what))
    ok = ~np.isnan(a)
    np.testing.assert_array_equal(a[ok].view(np.uint32), b[ok].view(np.uint32), err_msg=str(what))


@pytest.mark.parametrize("fmt", ["u8", "u16"])
@pytest.mark.parametrize("rng", hr.RANGES, ids=[f"{a:g}_{b:g}" for a, b in hr.RANGES])
def test_quantiser_against_the_reference(zfft_lib, fmt, rng):
    lo, hi = rng
    K, flo, _, step = hr.constants(fmt, lo, hi)
    what = (fmt, rng)
    # 100,000 seeded uniform values spanning 10 dB beyond both ends
    v = np.random.default_rng(K + int(abs(lo))).uniform(lo - 10.0, hi + 10.0, 100_000).astype(np.float32)
    # the specials, both end levels, and the half-step ties between neighbouring codes
    all_codes = np.arange(1, K + 2)
    levels = hr.unpack(all_codes, fmt, lo, hi)
    ties = (levels[:-1].astype(np.float64) + levels[1:].astype(np.float64)) / 2
    ties = ties[:: max(1, len(ties) // 2000)].astype(np.float32)
    special = np.float32([np.nan, np.inf, -np.inf, 0.0, -0.0, lo, hi, np.nextafter(np.float32(lo), np.float32(-np.inf)),
                          np.nextafter(np.float32(hi), np.float32(np.inf))])
    for vals in (v, special, ties, np.nextafter(ties, np.float32(np.inf)), np.nextafter(ties, np.float32(-np.inf))):
        ref = hr.pack(vals, fmt, lo, hi)
        np.testing.assert_array_equal(lib_codes(zfft_lib, fmt, lo, hi, vals), ref, err_msg=str(what))
        same_bits(lib_values(zfft_lib, fmt, lo, hi, ref), hr.unpack(ref, fmt, lo, hi), what)
    c = hr.pack(special, fmt, lo, hi)
    assert c[0] == 0 and c[1] == K + 1 and c[2] == 1 and c[5] == 1 and c[6] == K + 1 and c[7] == 1 and c[8] == K + 1, what
    assert np.isnan(hr.unpack([0], fmt, lo, hi)[0]) and hr.unpack([1], fmt, lo, hi)[0] == flo
    # every value of every code through the library
    same_bits(lib_values(zfft_lib, fmt, lo, hi, np.arange(0, K + 2)), hr.unpack(np.arange(0, K + 2), fmt, lo, hi), what)
    # the three properties, on the CPU reference: idempotence over every code ...
    np.testing.assert_array_equal(hr.pack(levels, fmt, lo, hi), all_codes, err_msg=str(what))
    assert (np.diff(levels) >= 0).all(), what
    # ... codes never decrease with v ...
    vs = np.sort(v)
    assert (np.diff(hr.pack(vs, fmt, lo, hi).astype(np.int64)) >= 0).all(), what
    # ... and the round trip inside the range stays within 0.513 step
    more = np.random.default_rng(K + 1).uniform(lo, hi, 100_000).astype(np.float32)  # (a narrow range holds few of v)
    inside = np.concatenate([vs, more, ties])
    inside = inside[(inside >= np.float32(lo)) & (inside <= np.float32(hi))]
    err = np.abs(hr.unpack(hr.pack(inside, fmt, lo, hi), fmt, lo, hi).astype(np.float64) - inside.astype(np.float64))
    assert len(inside) > 50_000 and err.max() <= 0.513 * float(step), (what, err.max() / float(step))


def test_quantiser_refuses_bad_arguments(zfft_lib):
    v, c = np.zeros(4, np.float32), np.zeros(4, np.uint16)
    for fmt, lo, hi in ((0, -150.0, -50.0), (3, -150.0, -50.0), (-1, -150.0, -50.0), (2, -50.0, -150.0), (2, 1.0, 1.0),
                        (1, float("nan"), 1.0), (2, -float("inf"), 1.0), (2, 0.0, float("inf"))):
        assert zfft_lib.zfft_history_codes(fmt, lo, hi, v.ctypes.data, 4, c.ctypes.data) == EINVAL, (fmt, lo, hi)
        assert zfft_lib.zfft_history_values(fmt, lo, hi, c.ctypes.data, 4, v.ctypes.data) == EINVAL, (fmt, lo, hi)
    assert zfft_lib.zfft_history_codes(2, -150.0, -50.0, v.ctypes.data, -1, c.ctypes.data) == EINVAL
    assert zfft_lib.zfft_history_codes(2, -150.0, -50.0, None, 4, c.ctypes.data) == EINVAL
    c[:] = 256  # above K + 1 for U8
    assert zfft_lib.zfft_history_values(2, -150.0, -50.0, c.ctypes.data, 4, v.ctypes.data) == EINVAL
    assert zfft_lib.zfft_history_values(1, -150.0, -50.0, c.ctypes.data, 4, v.ctypes.data) == 0


def test_ref_view_marks_lines_outside_the_store():
    kept = np.arange(7 * 8, dtype=np.float32).reshape(7, 8)  # rows 5 .. 11
    got = hr.ref_view(kept, 5, 8, 3, 6, (0, 8, 4), "max", 2)
    assert np.isnan(got[0]).all() and np.isnan(got[5]).all()  # rows 3, 4 and rows 13, 14
    np.testing.assert_array_equal(got[1], np.float32([9, 11, 13, 15]))  # rows 5, 6
    assert np.isnan(got[4]).all() and not np.isnan(got[3]).any()  # rows 11, 12: 12 is not there yet
    assert np.isnan(hr.ref_view(kept, 5, 8, -4, 2, (0, 8, 4), "mean", 2)).all()


FIELDS = ("kind", "px", "tiles", "lines", "k", "s", "slice_rows", "gy")
WHOLE, SLICED = 1, 2
TILE = {0: (256, 4), 1: (512, 8), 2: (1024, 16)}  # format: columns a wave loads per row, per lane


def history_form(lib, lines, m, span, width, fmt):
    """zfft__history_form as a dict of FIELDS, or None where the chooser refuses."""
    hook = lib.zfft__history_form
    hook.argtypes = [ctypes.c_int32] * 5 + [ctypes.POINTER(ctypes.c_int32)]
    hook.restype = ctypes.c_int
    out = (ctypes.c_int32 * 8)()
    return None if hook(lines, m, span, width, fmt, out) else dict(zip(FIELDS, out))


def test_form_chooser_sweep(zfft_lib):
    """Every form lies inside its own domain (what launch_history_view guards), and both forms --
    whole groups per workgroup, groups cut into slices -- are returned somewhere in the sweep."""
    seen = set()
    for fmt, lines, m, width, span in itertools.product((0, 1, 2), (1, 2, 37, 1080, 8192), (1, 5, 121, 3000, 65536),
                                                        (1, 16, 32, 1920), (2048, 8192, 65536)):
        f = history_form(zfft_lib, lines, m, span, width, fmt)
        what = (fmt, lines, m, span, width, f)
        assert f is not None, what
        bmax = -(-span // width)
        room = TILE[fmt][0] - (TILE[fmt][1] - 1)
        assert f["lines"] == lines, what
        assert f["px"] >= 1 and f["px"] * f["tiles"] >= width > f["px"] * (f["tiles"] - 1), what
        assert f["px"] == 1 or f["px"] * bmax <= room, what
        assert 1 <= f["tiles"] <= 65535 and f["gy"] >= 1, what
        if f["kind"] == WHOLE:
            assert f["s"] == 1 and f["k"] >= 1, what
            assert f["gy"] * f["k"] >= lines > (f["gy"] - 1) * f["k"], what
        else:
            assert f["kind"] == SLICED and f["k"] == 1 and lines * f["tiles"] < 512, what
            assert f["s"] >= 2 and f["s"] * f["slice_rows"] >= m > (f["s"] - 1) * f["slice_rows"], what
            assert f["slice_rows"] >= 32 and f["gy"] == lines * f["s"], what
        seen.add(f["kind"])
    assert seen == {WHOLE, SLICED}
    # a screenful of lines fills the chip with whole groups; two long lines are sliced
    f = history_form(zfft_lib, 1080, 121, 8192, 1920, 2)
    assert f["kind"] == WHOLE and f["gy"] * f["tiles"] >= 1024
    f = history_form(zfft_lib, 2, 3000, 128, 16, 2)
    assert f["kind"] == SLICED and f["gy"] * f["tiles"] >= 64
    assert history_form(zfft_lib, 2, 1, 128, 16, 2)["kind"] == WHOLE
    for bad in ((0, 1, 8, 8, 2), (8193, 1, 8, 8, 2), (1, 0, 8, 8, 2), (1, 65537, 8, 8, 2), (1, 1, 8, 9, 2),
                (1, 1, 8, 0, 2), (1, 1, 65537, 8, 2), (1, 1, 8, 8, 3), (1, 1, 8, 8, -1), (8192, 1, 8192, 4097, 2)):
        assert history_form(zfft_lib, *bad) is None, bad


def test_history_form_sweep_sanitized(tmp_path):
    """The chooser and the quantiser over their domains as a stand-alone g++ program (no HIP, no
    Python in the child) under AddressSanitizer + UBSan: tests/host/history_form_sweep.cpp."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/host/history_form_sweep.cpp"
    csrc = os.path.join(ROOT, "pypanadapter_amd", "csrc")
    exe = str(tmp_path / "history_form_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", csrc, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "history_form_sweep.cpp"),
                    os.path.join(csrc, "zfft_history_plan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "history_form_sweep: ok" in r.stdout, r.stdout
