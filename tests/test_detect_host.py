"""CPU checks of the row detector: the rule of include/zfft.h as detect_ref.ref_detect states it,
pinned clause by clause on hand-made rows; the C-ABI's new names; and the form chooser
(csrc/zfft_detect_plan.cpp) swept over its domain by a stand-alone program under ASan + UBSan."""
import ctypes
import os
import shutil
import subprocess

import numpy as np

import detect_ref as dr
from test_host import header_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["zfft_plan_detect", "zfft_detect_shape", "zfft_detect_device", "zfft_detect",
         "zfft_detect_occupancy", "zfft_detect_reset"]
NAN, INF = np.float32(np.nan), np.float32(np.inf)


def _one(row, **kw):
    row = np.asarray(row, dtype=np.float32)
    kw.setdefault("row_len", row.size)
    floor, found, events, occ = dr.ref_detect(row[None, :], **kw)
    return floor[0], int(found[0]), events[0], occ


def _runs(events, n):
    return [(int(e["first"]), int(e["last"]), int(e["peak"]), float(e["peak_db"])) for e in events[:n]]


def test_rank_formula_for_even_and_odd_m():
    """k = floor(q (m - 1)): q = 0 the minimum, q = 1 the maximum, q = 0.5 the lower median."""
    odd = [5.0, 1.0, 4.0, 2.0, 3.0]           # m = 5: k = 0, 2, 4
    even = [6.0, 5.0, 1.0, 4.0, 2.0, 3.0]     # m = 6: k = 0, 2 (2.5 floored), 5
    for row, want in ((odd, (1.0, 3.0, 5.0)), (even, (1.0, 3.0, 6.0))):
        for q, w in zip((0.0, 0.5, 1.0), want):
            assert _one(row, quantile=q, threshold_db=100.0)[0] == np.float32(w), (row, q)
    assert _one(even, quantile=0.25, threshold_db=100.0)[0] == np.float32(2.0)  # floor(1.25) = 1
    assert _one([7.0], quantile=0.7, threshold_db=100.0)[0] == np.float32(7.0)  # m = 1: k = 0


def test_population_leaves_out_nan_and_infinities():
    row = [NAN, -INF, 1.0, INF, 3.0, 2.0, NAN, -INF]
    floor, found, ev, occ = _one(row, quantile=0.5, threshold_db=1.0)  # m = 3, floor 2, thr 3
    assert floor == np.float32(2.0)
    # +inf is on, NaN and -inf are off: runs [3, 4] (peak the +inf at 3)
    assert found == 1 and _runs(ev, 1) == [(3, 4, 3, float("inf"))]
    np.testing.assert_array_equal(occ, [0, 0, 0, 1, 1, 0, 0, 0])
    # with the infinities counted the median would be another value
    assert _one([-INF, -INF, -INF, 1.0, 2.0], quantile=0.0, threshold_db=50.0)[0] == np.float32(1.0)
    assert _one([INF, INF, INF, 1.0, 2.0], quantile=1.0, threshold_db=50.0)[0] == np.float32(2.0)


def test_all_nan_row_has_nan_floor_and_no_emission():
    floor, found, ev, occ = _one([NAN, INF, -INF, NAN], threshold_db=-1000.0)
    assert np.isnan(floor) and found == 0 and not occ.any()
    assert ev.tobytes() == bytes(ev.nbytes)  # zero records


def test_threshold_edge_and_the_float_below():
    thr = np.float32(-100.0) + np.float32(12.0)
    below = np.nextafter(thr, np.float32(-np.inf), dtype=np.float32)
    row = np.array([-100.0] * 5 + [thr, -100.0, below, -100.0], dtype=np.float32)
    floor, found, ev, _ = _one(row, threshold_db=12.0)
    assert floor == np.float32(-100.0) and found == 1
    assert _runs(ev, 1) == [(5, 5, 5, float(thr))]
    # thr is one float32 addition: 0.1 is rounded to float32 first, then the sum once
    f = np.float32(-77.7)
    row = np.array([f, f, f, np.float32(f + np.float32(0.1))], dtype=np.float32)
    assert _one(row, threshold_db=0.1)[1] == 1
    # a negative threshold: everything at or above floor - 3 is on, one run
    row = np.array([-100.0, -101.0, -102.0, -104.0, -100.0, -99.0, -100.5], dtype=np.float32)
    floor, found, ev, _ = _one(row, threshold_db=-3.0)  # floor -100.5 (k = 3), thr -103.5
    assert floor == np.float32(-100.5) and found == 2
    assert _runs(ev, 2) == [(0, 2, 0, -100.0), (4, 6, 5, -99.0)]


def test_runs_at_both_ends_and_min_width():
    lo, hi = -100.0, -50.0
    row = np.full(24, lo, dtype=np.float32)
    row[0:2] = hi        # touches column 0, width 2
    row[5:8] = hi        # width 3
    row[10:14] = hi      # width 4
    row[21:24] = hi      # touches the last column, width 3
    for mw, want in ((1, [(0, 1), (5, 7), (10, 13), (21, 23)]), (3, [(5, 7), (10, 13), (21, 23)]),
                     (4, [(10, 13)]), (5, [])):
        floor, found, ev, occ = _one(row, threshold_db=12.0, min_width=mw)
        assert floor == np.float32(lo) and found == len(want), mw
        assert [(a, b) for a, b, _, _ in _runs(ev, found)] == want, mw
        ref_occ = np.zeros(24, dtype=np.uint32)
        for a, b in want:
            ref_occ[a:b + 1] = 1
        np.testing.assert_array_equal(occ, ref_occ)
    # gaps are not bridged: one off column splits a run, and both halves may fall short
    row = np.full(24, lo, dtype=np.float32)
    row[4:6] = hi
    row[7:9] = hi
    assert _one(row, min_width=1)[1] == 2 and _one(row, min_width=3)[1] == 0


def test_cap_counts_every_run_and_records_the_first_k():
    row = np.full(40, -100.0, dtype=np.float32)
    row[1::4] = -40.0  # 10 runs of one column at 1, 5, ..., 37
    floor, found, ev, occ = _one(row, K=3)
    assert found == 10 and _runs(ev, 3) == [(1, 1, 1, -40.0), (5, 5, 5, -40.0), (9, 9, 9, -40.0)]
    assert occ.sum() == 10 and np.all(occ[1::4] == 1)  # the runs beyond the cap count too
    _, found, ev, _ = _one(row, K=32)
    assert found == 10 and ev[10:].tobytes() == bytes(ev[10:].nbytes)  # the unused slots are zero records


def test_peak_ties_go_to_the_lowest_column_and_keep_the_bits():
    row = np.array([-9.0] * 6 + [5.0, 7.0, 7.0, 6.0] + [-9.0] * 2, dtype=np.float32)
    assert _runs(_one(row)[2], 1) == [(6, 9, 7, 7.0)]
    # -0.0 and 0.0 are equal: the first of them is the peak, sign and all
    row = np.array([-50.0] * 5 + [-0.0, 0.0, -50.0], dtype=np.float32)
    ev = _one(row)[2]
    assert int(ev[0]["peak"]) == 5 and np.signbit(ev[0]["peak_db"])
    row = np.array([-50.0] * 5 + [0.0, -0.0, -50.0], dtype=np.float32)
    ev = _one(row)[2]
    assert int(ev[0]["peak"]) == 5 and not np.signbit(ev[0]["peak_db"])


def test_tail_columns_are_not_read_and_occupancy_sums_over_rows():
    rows = np.full((3, 8), -100.0, dtype=np.float32)
    rows[:, 6:] = 1e30    # beyond row_len = 6: neither in the floor nor an emission
    rows[0, 2] = rows[1, 2] = rows[1, 3] = -60.0
    floor, found, events, occ = dr.ref_detect(rows, 6, 1.0 / 3.0, 12.0, 1, 2)
    np.testing.assert_array_equal(floor, np.float32([-100.0] * 3))
    np.testing.assert_array_equal(found, [1, 1, 0])
    np.testing.assert_array_equal(occ, [0, 0, 2, 1, 0, 0, 0, 0])
    assert occ.dtype == np.uint32 and events.shape == (3, 2) and events.dtype.itemsize == 16


def test_new_names_are_declared_and_exported(zfft_lib):
    from pypanadapter_amd import _lib
    declared = header_functions()
    for name in NAMES:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert getattr(zfft_lib, name).argtypes is not None, name


def detect_form(lib, row_len, count):
    """(waves, per, grid) of zfft__detect_form, or None where it refuses."""
    hook = lib.zfft__detect_form
    hook.argtypes = [ctypes.c_int32, ctypes.c_int32] + [ctypes.POINTER(ctypes.c_int32)] * 3
    hook.restype = ctypes.c_int
    w, p, g = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    rc = hook(row_len, count, ctypes.byref(w), ctypes.byref(p), ctypes.byref(g))
    return None if rc else (w.value, p.value, g.value)


def test_form_chooser_through_the_hook(zfft_lib):
    """The narrow rows (the UI's and cfg2's) take one wave per row; every width up to 65,536 has
    a form that holds it, and the grid never exceeds the rows."""
    for n in (1, 50, 64):
        assert detect_form(zfft_lib, n, 37)[:2] == (1, 1)
    assert detect_form(zfft_lib, 151, 37)[:2] == (1, 4)
    assert detect_form(zfft_lib, 512, 69632)[:2] == (1, 8)
    assert detect_form(zfft_lib, 513, 37)[0] > 1
    for n in (1, 63, 64, 65, 128, 129, 256, 257, 512, 513, 2048, 2049, 8192, 8193, 65535, 65536):
        for count in (1, 3, 37, 69632, 1 << 26):
            w, p, g = detect_form(zfft_lib, n, count)
            assert 64 * w * p >= n and 1 <= g <= count and w in (1, 4, 16), (n, count)
    for bad in ((0, 1), (65537, 1), (64, 0), (-1, 5), (64, -3)):
        assert detect_form(zfft_lib, *bad) is None, bad


def test_detect_form_sweep_sanitized(tmp_path):
    """The chooser over every row_len in [1, 65536] as a stand-alone g++ program (no HIP, no
    Python in the child) under AddressSanitizer + UBSan: tests/host/detect_form_sweep.cpp."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/host/detect_form_sweep.cpp"
    csrc = os.path.join(ROOT, "pypanadapter_amd", "csrc")
    exe = str(tmp_path / "detect_form_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", csrc, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "detect_form_sweep.cpp"),
                    os.path.join(csrc, "zfft_detect_plan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "detect_form_sweep: ok" in r.stdout, r.stdout


def test_meaning_case_input_condition(oracle_lib):
    """The input of test_gpu_detect.py's planted-tone test, checked without a GPU: on the oracle's
    float64 rows the rule finds exactly the three tones, at their bins, the weakest about 30 units
    over the floor, and no reference value lies within 0.01 units of the threshold (ten times the
    row gate DB_TOL), so a device row inside the gate has the same columns on."""
    import welch_average_ref as war
    c = dr.MEANING
    x = dr.meaning_frames()
    ref_rows = np.stack([war.ref_row(x[f], c["fs"], c["N"], c["zoom"], c["W"], "mean") for f in range(c["F"])])
    floor64 = np.sort(ref_rows, axis=1)[:, (c["W"] - 1) // 2]
    assert np.abs(ref_rows - (floor64 + c["threshold_db"])[:, None]).min() > 0.01
    floor, found, ev, occ = dr.ref_detect(ref_rows.astype(np.float32), c["W"], 0.5, c["threshold_db"], 1, 8)
    np.testing.assert_array_equal(found, [3] * c["F"])
    for f in range(c["F"]):
        for r, (b, _) in enumerate(c["tones"]):
            assert ev[f, r]["peak"] == c["W"] // 2 + b and ev[f, r]["first"] <= ev[f, r]["peak"] <= ev[f, r]["last"]
        assert 27.0 < ev[f, 0]["peak_db"] - floor[f] < 33.0
        assert ev[f, 0]["peak_db"] < ev[f, 1]["peak_db"] < ev[f, 2]["peak_db"]
