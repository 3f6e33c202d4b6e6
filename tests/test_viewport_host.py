"""CPU checks of the display viewport: the rule of include/zfft.h as viewport_ref states it,
pinned on hand-made values; zfft_viewport_edge against it; the declared and exported names; and
the pure form chooser (zfft_view_plan.h) swept through its hook.  No call reaches a GPU here."""
import ctypes
import itertools
import os
import shutil
import subprocess

import numpy as np

from conftest import ROOT

import viewport_ref as vr
from test_host import header_functions

NAMES = ["zfft_plan_viewport", "zfft_viewport_edge", "zfft_viewport_shape", "zfft_viewport_push_device",
         "zfft_viewport_push", "zfft_viewport_state", "zfft_viewport_read", "zfft_viewport_traces",
         "zfft_viewport_hold_reset", "zfft_viewport_reset", "zfft_viewport_render_device",
         "zfft_viewport_render", "zfft_viewport_push_render"]
NAN, INF = np.nan, np.inf


def test_ref_on_hand_made_values():
    # 10 columns, the window [2, 9) into 3 pixels: edges 2, 4, 6, 9
    np.testing.assert_array_equal(vr.edges(2, 9, 3), [2, 4, 6, 9])
    rows = np.float32([[9e9, 9e9, -10, -20, NAN, -30, -50, -40, -60, 9e9],
                       [9e9, 9e9, -15, -5, NAN, NAN, -INF, -70, -45, 9e9]])
    g = (2, 9, 3)
    mx, pend = vr.ref_lines(rows, 9, g, "max", 1)
    np.testing.assert_array_equal(mx, np.float32([[-10, -30, -40], [-5, NAN, -45]]))
    assert mx.dtype == np.float32 and pend[0] == 0
    mn, _ = vr.ref_lines(rows, 9, g, "min", 2)
    np.testing.assert_array_equal(mn, np.float32([[-20, -30, -INF]]))
    # mean: pixel 0 of both rows = the mean of 10^(-10/20), 10^(-20/20), 10^(-15/20), 10^(-5/20)
    me, _ = vr.ref_lines(rows, 9, g, "mean", 2)
    want = 20 * np.log10((10 ** -0.5 + 10 ** -1.0 + 10 ** -0.75 + 10 ** -0.25) / 4)
    assert me.dtype == np.float64 and abs(me[0, 0] - want) < 1e-12
    assert np.isnan(me[0, 1])  # any NaN in the cell
    # -inf contributes 0: five finite values and one zero over 6 cells
    want2 = 20 * np.log10((10 ** -2.5 + 10 ** -2.0 + 10 ** -3.0 + 10 ** -3.5 + 10 ** -2.25) / 6)
    assert abs(me[0, 2] - want2) < 1e-12
    allz, _ = vr.ref_lines(np.full((1, 4), -INF, np.float32), 4, (0, 4, 2), "mean", 1)
    np.testing.assert_array_equal(allz, [[-INF, -INF]])
    pinf, _ = vr.ref_lines(np.float32([[INF, -3, -3, -3]]), 4, (0, 4, 2), "mean", 1)
    assert pinf[0, 0] == INF and abs(pinf[0, 1] + 3) < 1e-12


def test_ref_groups_do_not_depend_on_the_split():
    rng = np.random.default_rng(3)
    rows = rng.uniform(-160, -40, (25, 16)).astype(np.float32)
    g = (1, 15, 5)
    for det in vr.DETECTORS:
        whole, pend = vr.ref_lines(rows, 16, g, det, 5)
        assert whole.shape == (5, 5) and pend[0] == 0
        got, state, at = [], None, 0
        for cnt, left in ((1, 1), (3, 4), (7, 1), (4, 0), (10, 0)):
            lines, state = vr.ref_lines(rows[at:at + cnt], 16, g, det, 5, state)
            at += cnt
            got.append(lines)
            assert state[0] == left
        got = np.concatenate(got)
        if det == "mean":
            np.testing.assert_allclose(got, whole, rtol=0, atol=1e-11)
        else:
            np.testing.assert_array_equal(got, whole)


def test_ref_image_and_holds():
    lines = np.float32([[1, 5], [2, 4], [3, NAN]])
    up = vr.ref_image(lines, 4, +1)
    np.testing.assert_array_equal(up, np.float32([[NAN, NAN], [1, 5], [2, 4], [3, NAN]]))
    down = vr.ref_image(lines, 2, -1)
    np.testing.assert_array_equal(down, np.float32([[3, NAN], [2, 4]]))
    last, mx, mn = vr.ref_holds(lines)
    np.testing.assert_array_equal(last, lines[2])
    np.testing.assert_array_equal(mx, np.float32([3, 5]))
    np.testing.assert_array_equal(mn, np.float32([1, 4]))
    last0, mx0, _ = vr.ref_holds(lines[:0].reshape(0, 2))
    assert np.isnan(last0).all() and np.isnan(mx0).all()


def test_plant_specials_and_poison():
    g = (5, 150, 7)
    rows = np.random.default_rng(1).uniform(-160, -40, (5, 301)).astype(np.float32)
    assert vr.plant_specials(rows, g, 2) > 10
    vr.poison_outside(rows, 151, g)
    assert not np.isfinite(rows[:, :5]).all() and (rows[:, 150:] != rows[:, 150:]).any()
    mx, _ = vr.ref_lines(rows, 151, g, "max", 2)
    assert np.isnan(mx[0, 1]) and mx[0, 6] == -INF and np.isfinite(mx[1]).sum() >= 5
    assert (mx[np.isfinite(mx)] <= 0).all()  # the planted zeros at most: no poison reached a cell
    me, _ = vr.ref_lines(rows, 151, g, "mean", 2)
    assert me[0, 6] == -INF and np.isnan(me[0, 1])


def _edge(lib, *a):
    return lib.zfft_viewport_edge(*a)


def test_viewport_edge_against_the_ref(zfft_lib):
    for col0, col1, width in ((0, 512, 512), (3, 500, 7), (0, 8192, 1920), (10, 74, 64), (0, 65536, 1)):
        e = vr.edges(col0, col1, width)
        got = [_edge(zfft_lib, col0, col1, width, x) for x in range(width + 1)]
        np.testing.assert_array_equal(got, e)
        d = np.diff(e)
        assert e[0] == col0 and e[-1] == col1 and d.min() >= 1 and d.max() - d.min() <= 1
    assert sorted(set(np.diff(vr.edges(0, 8192, 1920)))) == [4, 5]
    for bad in ((-1, 8, 4, 0), (4, 4, 1, 0), (8, 4, 2, 0), (0, 8, 0, 0), (0, 8, 9, 0), (0, 8, 4, -1), (0, 8, 4, 5)):
        assert _edge(zfft_lib, *bad) == -1, bad


def test_new_names_are_declared_and_exported(zfft_lib):
    from pypanadapter_amd import _lib
    declared = header_functions()
    for name in NAMES:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert getattr(zfft_lib, name).argtypes is not None, name
    assert _lib.VIEW_DETECTORS == {"max": 0, "min": 1, "mean": 2}


FIELDS = ("kind", "team", "px", "tiles", "groups", "k", "s", "slice_rows", "gy")
LINES, SPLIT = 1, 2


def view_form(lib, count, m, pending, span, width):
    """zfft__view_form as a dict of FIELDS, or None where the chooser refuses."""
    hook = lib.zfft__view_form
    hook.argtypes = [ctypes.c_int32] * 5 + [ctypes.POINTER(ctypes.c_int32)]
    hook.restype = ctypes.c_int
    out = (ctypes.c_int32 * 9)()
    return None if hook(count, m, pending, span, width, out) else dict(zip(FIELDS, out))


def test_form_chooser_sweep(zfft_lib):
    """Every form lies inside its own domain (what launch_view_lines guards), and each form the
    chooser has -- lines with a team of four waves, lines with one wave per group, split -- is
    returned somewhere in the sweep."""
    seen = set()
    for count, m, width, span in itertools.product((1, 37, 7000, 69632), (1, 5, 3000, 65536), (1, 32, 1920),
                                                   (2048, 8192, 65536)):
        for pending in sorted({0, m // 2, m - 1}):
            f = view_form(zfft_lib, count, m, pending, span, width)
            what = (count, m, pending, span, width, f)
            assert f is not None, what
            bmax = -(-span // width)
            groups = -(-(pending + count) // m)
            assert f["groups"] == groups, what
            assert f["px"] >= 1 and f["px"] * f["tiles"] >= width > f["px"] * (f["tiles"] - 1), what
            assert f["px"] == 1 or f["px"] * bmax <= 256, what
            assert 1 <= f["tiles"] <= 65535 and f["gy"] >= 1, what
            if f["kind"] == LINES:
                assert f["s"] == 1 and f["team"] in (1, 4) and f["k"] >= 1, what
                assert f["gy"] * f["k"] >= groups > (f["gy"] - 1) * f["k"], what
                assert f["team"] == 4 or f["k"] % 4 == 0, what
                assert (f["team"] == 4) == (m >= 16), what
            else:
                assert f["kind"] == SPLIT and f["team"] == 4 and f["k"] == 1, what
                assert f["s"] >= 2 and f["s"] * f["slice_rows"] >= m > (f["s"] - 1) * f["slice_rows"], what
                assert f["slice_rows"] >= 32 and f["gy"] == groups * f["s"], what
            seen.add((f["kind"], f["team"]))
    assert seen == {(LINES, 4), (LINES, 1), (SPLIT, 4)}
    # the streaming case fills the chip with whole groups; one long group is split
    f = view_form(zfft_lib, 69632, 64, 0, 512, 256)
    assert f["kind"] == LINES and f["team"] == 4 and f["gy"] * f["tiles"] >= 1024
    f = view_form(zfft_lib, 65536, 65536, 0, 512, 256)
    assert f["kind"] == SPLIT and f["gy"] * f["tiles"] >= 512
    assert view_form(zfft_lib, 7000, 3000, 0, 128, 32)["kind"] == SPLIT
    for bad in ((0, 1, 0, 8, 8), (1, 0, 0, 8, 8), (1, 65537, 0, 8, 8), (1, 5, 5, 8, 8), (1, 5, -1, 8, 8),
                (1, 1, 0, 8, 9), (1, 1, 0, 8, 0), (1, 1, 0, 65537, 8)):
        assert view_form(zfft_lib, *bad) is None, bad


def test_view_form_sweep_sanitized(tmp_path):
    """The chooser and the bucket edge over their domains as a stand-alone g++ program (no HIP, no
    Python in the child) under AddressSanitizer + UBSan: tests/host/view_form_sweep.cpp."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/host/view_form_sweep.cpp"
    csrc = os.path.join(ROOT, "pypanadapter_amd", "csrc")
    exe = str(tmp_path / "view_form_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", csrc, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "view_form_sweep.cpp"),
                    os.path.join(csrc, "zfft_view_plan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "view_form_sweep: ok" in r.stdout, r.stdout
