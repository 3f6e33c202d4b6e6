"""CPU checks of the detector's local floor (zfft_plan_detect_local): the C-ABI's new names, the
reference rule's own properties (tests/detect_local_ref.py), the input condition of the GPU
"meaning" test from the references alone, and the form chooser (csrc/zfft_detect_plan.cpp) swept
through its hook and by a stand-alone program under ASan + UBSan."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import detect_local_ref as dl
import detect_ref as dr
from test_host import header_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["zfft_plan_detect_local", "zfft_detect_local_shape", "zfft_detect_floors_device", "zfft_detect_floors"]


def test_new_names_are_declared_and_exported(zfft_lib):
    from pypanadapter_amd import _lib
    declared = header_functions()
    for name in NAMES:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert getattr(zfft_lib, name).argtypes is not None, name
    from pypanadapter_amd import ZoomFFT, panadapter
    for name in ("set_detect_local", "detect_local_shape", "detect_floors", "detect_floors_device"):
        assert callable(getattr(ZoomFFT, name)), name
    assert callable(panadapter.Detector.floors)


# ---------------------------------------------------------------- the reference's own properties
@pytest.mark.parametrize("n,h,gd", [(1, 1, 0), (7, 2, 1), (50, 16, 2), (50, 128, 128), (300, 128, 128), (64, 1, 0)])
def test_window_never_holds_the_column_or_its_guards(n, h, gd):
    for j in range(n):
        c = dl.window_columns(j, n, h, gd)
        assert np.all((c >= 0) & (c < n)) and np.all(np.diff(c) > 0)
        d = np.abs(c - j)
        assert np.all((d > gd) & (d <= gd + h))
        want = [k for k in range(n) if gd < abs(k - j) <= gd + h]
        assert c.tolist() == want
    if n <= gd + 1:
        assert all(dl.window_columns(j, n, h, gd).size == 0 for j in range(n))


def test_a_constant_row_gives_the_constant_everywhere():
    for val in (-97.25, 0.0, 3.5e-42):
        row = np.full((1, 40), val, dtype=np.float32)
        for h, gd in ((1, 0), (16, 2), (128, 128)):
            for q in (0.0, 0.5, 1.0):
                fl = dl.ref_local_floors(row, 40, h, gd, q)[0]
                if gd + 1 >= 40:
                    assert np.all(np.isnan(fl))
                else:
                    lone = np.array([dl.window_columns(j, 40, h, gd).size == 0 for j in range(40)])
                    assert np.all(fl[~lone] == np.float32(val)) and np.all(np.isnan(fl[lone]))


def test_a_window_wider_than_the_row_is_the_order_statistic_of_all_other_columns():
    rng = np.random.default_rng(11)
    n = 37
    v = rng.permutation(n).astype(np.float32)  # all distinct
    for h in (37, 64, 128):
        for q in (0.0, 0.3, 0.5, 1.0):
            fl = dl.ref_local_floors(v[None, :], n, h, 0, q)[0]
            for j in range(n):
                others = np.sort(np.delete(v, j))
                assert fl[j] == others[int(np.floor(q * float(n - 2)))]


def test_population_leaves_out_non_finite_cells_and_empty_windows_are_nan():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    row = np.array([[1.0, nan, inf, 5.0, -inf, 2.0, 9.0, nan]], dtype=np.float32)
    fl = dl.ref_local_floors(row, 8, 2, 0, 1.0)[0]
    #        j:   0 {1,2}->none; 1 {0,2,3}->max(1,5); 2 {0,1,3,4}->5; 3 {1,2,4,5}->2; 4 {2,3,5,6}->9
    assert np.isnan(fl[0]) and fl[1] == 5.0 and fl[2] == 5.0 and fl[3] == 2.0 and fl[4] == 9.0
    # +inf is left out of the floor but is itself on; a NaN floor keeps its column off
    floor, found, ev, occ = dl.ref_detect_local(row, 8, 2, 0, 1.0, -100.0, 1, 8)
    assert occ[0] == 0 and occ[2] == 1 and occ[1] == 0 and occ[4] == 0
    # the tail beyond row_len is neither a reference cell nor written
    row2 = np.array([[1.0, 2.0, 3.0, 1e30, 1e30]], dtype=np.float32)
    fl2 = dl.ref_local_floors(row2, 3, 4, 0, 1.0)[0]
    assert fl2[:3].tolist() == [3.0, 3.0, 2.0] and np.all(np.isnan(fl2[3:]))


def test_the_vectorised_reference_is_the_loop():
    rng = np.random.default_rng(5)
    rows = (-120.0 + 3.0 * rng.standard_normal((3, 70))).astype(np.float32)
    rows[:, 10:14] = np.nan
    rows[0, 30] = np.inf
    rows[1, 31:36] = -np.inf
    rows[2, :] = np.round(rows[2, :])  # ties
    rows[:, 66:] = 1e30
    for n in (1, 5, 66):
        for h, gd in ((1, 0), (3, 1), (16, 2), (128, 128), (128, 0)):
            for q in (0.0, 0.5, 0.75, 1.0):
                a, b = dl.ref_local_floors(rows, n, h, gd, q), dl.fast_local_floors(rows, n, h, gd, q)
                np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=str((n, h, gd, q)))


def test_local_detect_equals_global_detect_on_a_hand_made_row():
    """The run, record and occupancy code is detect_ref's: with floors handed in that are all the
    row's global floor, ref_detect_local is ref_detect."""
    rng = np.random.default_rng(8)
    rows = (-120.0 + rng.standard_normal((4, 64))).astype(np.float32)
    rows[:, 5:8] = -60.0
    rows[:, 30] = np.inf
    rows[:, 40:42] = np.nan
    rows[:, 63] = -70.0
    for mw, K in ((1, 8), (3, 2)):
        want = dr.ref_detect(rows, 64, 0.5, 12.0, mw, K)
        floors = np.repeat(want[0][:, None], 64, axis=1)
        got = dl.ref_detect_local(rows, 64, 4, 1, 0.5, 12.0, mw, K, floors=floors)
        dr.assert_same(got[:3], want[:3])
        np.testing.assert_array_equal(got[3], want[3])


# ---------------------------------------------------------------- meaning, from the references alone
def test_meaning_case_input_condition():
    """A floor rising 40 units over the row: the local rule finds exactly the planted tones (the
    device's rule is the reference's bit for bit, so no margin is needed); the global rule at q = 0.5 reports 21
    and 6 runs, misses the two tones in the quiet part and ends in one run up to the last column."""
    c = dl.MEANING_LOCAL
    for n, tones in c["rows"]:
        v = dl.meaning_row(n, tones)[None, :]
        _, gfound, gev, _ = dr.ref_detect(v, n, 0.5, c["threshold_db"], c["min_width"], c["K"])
        assert gfound[0] == c["global_runs"][n]
        runs = [(int(e["first"]), int(e["last"])) for e in gev[0, :gfound[0]]]
        for t in c["global_misses"][n]:
            assert not any(a <= t + 1 and b >= t for a, b in runs), t
        assert runs[-1][1] == n - 1
        for h, gd, q in c["shapes"]:
            _, found, ev, occ = dl.ref_detect_local(v, n, h, gd, q, c["threshold_db"], c["min_width"], c["K"])
            assert found[0] == len(tones), (n, h, gd, q)
            assert [(int(e["first"]), int(e["last"])) for e in ev[0, :found[0]]] == [(t, t + 1) for t in tones]
            assert all(t <= int(e["peak"]) <= t + 1 for e, t in zip(ev[0], tones))
            assert int(occ.sum()) == 2 * len(tones)


# ---------------------------------------------------------------- the form chooser
def local_form(lib, row_len, n_win, count, h, gd, scratch=0):
    """zfft__detect_local_form as a dict, or None where it refuses."""
    hook = lib.zfft__detect_local_form
    hook.argtypes = [ctypes.c_int32] * 5 + [ctypes.c_int64, ctypes.POINTER(ctypes.c_int32)]
    hook.restype = ctypes.c_int
    out = (ctypes.c_int32 * 7)()
    if hook(row_len, n_win, count, h, gd, scratch, out):
        return None
    return dict(zip(("tile", "tiles", "halo", "grid", "chunk_rows", "lds_keys", "words"), out))


def test_local_form_chooser_through_the_hook(zfft_lib):
    for n in (1, 50, 255, 256, 257, 512, 2049, 8192, 65535, 65536):
        for h in (1, 16, 32, 33, 64, 65, 128):
            for gd in (0, 128):
                for count in (1, 3, 69632, 1 << 26):
                    f = local_form(zfft_lib, n, n + (n & 1), count, h, gd)
                    assert f["tile"] == 256 and (f["tiles"] - 1) * 256 < n <= f["tiles"] * 256
                    assert f["halo"] == h + gd and f["lds_keys"] == 256 + 2 * (h + gd) and f["lds_keys"] <= 768
                    assert f["words"] == (1 if h <= 32 else 2 if h <= 64 else 4)
                    assert 1 <= f["chunk_rows"] <= count and f["chunk_rows"] * (n + (n & 1)) * 4 <= 256 << 20
                    assert 1 <= f["grid"] <= min(f["chunk_rows"] * f["tiles"], 1 << 16)
    # a small scratch: rows per pass follow it; less than a row is refused
    assert local_form(zfft_lib, 512, 512, 300, 16, 2, 512 * 4 * 7)["chunk_rows"] == 7
    assert local_form(zfft_lib, 512, 512, 300, 16, 2, 512 * 4 - 1) is None
    for bad in ((0, 2, 1, 1, 0), (3, 2, 1, 1, 0), (65537, 65538, 1, 1, 0), (64, 64, 0, 1, 0), (64, 64, 1, 0, 0),
                (64, 64, 1, 129, 0), (64, 64, 1, 1, -1), (64, 64, 1, 1, 129)):
        assert local_form(zfft_lib, *bad) is None, bad


def test_detect_local_form_sweep_sanitized(tmp_path):
    """The chooser over every row_len in [1, 65536] x h in {1, 16, 32, 33, 64, 65, 128} x guard in {0, 128} as a
    stand-alone g++ program (no HIP, no Python in the child) under AddressSanitizer + UBSan:
    tests/host/detect_local_form_sweep.cpp."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/host/detect_local_form_sweep.cpp"
    csrc = os.path.join(ROOT, "pypanadapter_amd", "csrc")
    exe = str(tmp_path / "detect_local_form_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", csrc, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "detect_local_form_sweep.cpp"),
                    os.path.join(csrc, "zfft_detect_plan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "detect_local_form_sweep: ok" in r.stdout, r.stdout
