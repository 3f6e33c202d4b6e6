"""The row detector's rule (include/zfft.h, zfft_plan_detect) in numpy float32, a plain loop.

A row is the first `row_len` floats of a stride of n_win; values are in row units (20 log10).
1. population: the finite values; NaN, +inf, -inf left out; m of them.  m == 0: floor = NaN, no
   emissions.
2. floor: np.sort(finite)[k], k = int(floor(q * float(m - 1))): one of the row's own values.
3. thr = floor + float32(threshold_db), one float32 addition; column j is on when v[j] >= thr
   (+inf on; NaN and -inf off).
4. an emission is a maximal run [first, last] of on columns with last - first + 1 >= min_width.
5. record (first, last, peak, peak_db): peak the lowest column holding the run's maximum,
   peak_db that value unchanged.
6. per row: floor, found = all kept runs, events = the first min(found, K) in column order, the
   other slots zero records.
7. occ[j] += 1 for every column of every kept run (recorded or not); uint32, n_win long.
"""
import numpy as np

EMISSION = np.dtype([("first", np.int32), ("last", np.int32), ("peak", np.int32), ("peak_db", np.float32)])


def ref_detect(rows, row_len, quantile=0.5, threshold_db=12.0, min_width=1, K=8):
    """(floor float32[count], found int32[count], events EMISSION[count, K], occ uint32[n_win])."""
    rows = np.asarray(rows, dtype=np.float32)
    rows = rows.reshape(-1, rows.shape[-1])
    count, n_win = rows.shape
    floor = np.full(count, np.nan, dtype=np.float32)
    found = np.zeros(count, dtype=np.int32)
    events = np.zeros((count, K), dtype=EMISSION)
    occ = np.zeros(n_win, dtype=np.uint32)
    add = np.float32(threshold_db)
    for i in range(count):
        v = rows[i, :row_len]
        fin = v[np.isfinite(v)]
        m = fin.size
        if m == 0:
            continue
        k = int(np.floor(quantile * float(m - 1)))
        floor[i] = np.sort(fin)[k]
        with np.errstate(over="ignore", invalid="ignore"):
            thr = np.float32(floor[i] + add)
            on = v >= thr
        edge = np.diff(np.concatenate(([0], on.astype(np.int8), [0])))
        first, last = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1) - 1
        keep = last - first + 1 >= min_width
        first, last = first[keep], last[keep]
        found[i] = first.size
        for r, (a, b) in enumerate(zip(first, last)):
            occ[a:b + 1] += np.uint32(1)
            if r < K:
                pk = a + int(np.argmax(v[a:b + 1]))
                events[i, r] = (a, b, pk, v[pk])
    return floor, found, events, occ


def assert_same(got, want):
    """(floor, found, events) compared exactly; peak_db as bits."""
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    for name in ("first", "last", "peak"):
        np.testing.assert_array_equal(got[2][name], want[2][name], err_msg=name)
    np.testing.assert_array_equal(np.ascontiguousarray(got[2]["peak_db"]).view(np.uint32),
                                  np.ascontiguousarray(want[2]["peak_db"]).view(np.uint32), err_msg="peak_db bits")


# ---- the planted-tone case of test_gpu_detect.py's "meaning" test (its input condition is
# checked without a GPU by test_detect_host.py): dif1024_nseg17's shape, one mean row per frame
MEANING = {"N": 1024, "zoom": 1, "W": 1024, "L": 9216, "F": 3, "fs": 2.4e6, "seed": 20260,
           "threshold_db": 12.0,  # 4x in power
           # (FFT bin from the centre, amplitude) over unit-variance complex noise: a Hamming
           # window's processing gain is 57.5 row units at amplitude 1, so 0.2 stands about 30
           # units over the floor
           "tones": ((-300, 0.2), (57, 0.7), (410, 2.5))}


def meaning_frames():
    """(F, L) complex64: seeded noise and three complex tones at exact bin frequencies."""
    c = MEANING
    rng = np.random.default_rng(c["seed"])
    x = (rng.standard_normal((c["F"], c["L"])) + 1j * rng.standard_normal((c["F"], c["L"]))) / np.sqrt(2.0)
    n = np.arange(c["L"])
    for b, a in c["tones"]:
        x = x + a * np.exp(2j * np.pi * b * n / c["N"])
    return x.astype(np.complex64)
