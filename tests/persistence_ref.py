"""The persistence spectrum's binning rule (include/zfft.h, zfft_plan_persistence) in numpy
float32, shared by tests/test_persistence_host.py (CPU: the rule pinned on hand-made values) and
tests/test_gpu_persistence.py (the device's table must equal it as integers).

    lo  = float32(db_min)
    inv = float32(levels / (db_max - db_min))     the division in double, rounded once
    t   = (v - lo) * inv                          float32 arrays: each operation rounded
    v counts in hist[int(t), column] when t >= 0 and t < levels; NaN, +-inf and levels outside
    the range count nowhere; columns >= row_length are never read."""
import numpy as np


def ref_hist(rows_f32, levels, db_min, db_max, row_length):
    """(levels, n_win) uint32 table of rows_f32 (count, n_win) float32."""
    rows = np.asarray(rows_f32)
    assert rows.dtype == np.float32 and rows.ndim == 2
    lo = np.float32(db_min)
    inv = np.float32(float(levels) / (float(db_max) - float(db_min)))
    with np.errstate(invalid="ignore", over="ignore"):
        t = (rows[:, :row_length] - lo) * inv
        assert t.dtype == np.float32
        ok = (t >= 0) & (t < levels)  # before the cast: NaN and inf have no integer
    hist = np.zeros((levels, rows.shape[1]), dtype=np.uint32)
    r, j = np.nonzero(ok)
    np.add.at(hist, (t[r, j].astype(np.int64), j), 1)
    return hist


# The rule's edge values for lo = -100, 8 levels of 5 dB (db_max = -60): value -> level, None =
# counted nowhere.  -60 is db_max itself; nextafter(-60, -inf) the largest float32 below it.
EDGE_LEVELS, EDGE_MIN, EDGE_MAX = 8, -100.0, -60.0
EDGE_VALUES = [
    (-100.0, 0), (-95.0, 1), (-90.0, 2), (-85.0, 3), (-80.0, 4), (-75.0, 5), (-70.0, 6), (-65.0, 7),
    (-60.0, None), (float(np.nextafter(np.float32(-60.0), np.float32(-np.inf))), 7),
    (float("nan"), None), (float("inf"), None), (float("-inf"), None), (-0.0, None),
    (float(np.nextafter(np.float32(-100.0), np.float32(-np.inf))), None),
]


def plant_edges(rows, levels, db_min, db_max, row_length):
    """Overwrite the head of `rows` (in place) with every edge of the given binning -- db_min,
    each interior edge, db_max, the floats next to db_min and db_max, NaN, +-inf, -0.0 -- one
    per cell, walking the columns < row_length row by row; returns how many were planted."""
    lo, hi = np.float32(db_min), np.float32(db_max)
    edges = [np.float32(db_min + (db_max - db_min) * k / levels) for k in range(levels + 1)]
    vals = edges + [np.nextafter(hi, np.float32(-np.inf)), np.nextafter(lo, np.float32(-np.inf)),
                    np.float32("nan"), np.float32("inf"), np.float32("-inf"), np.float32(-0.0)]
    n = min(len(vals), rows.shape[0] * row_length)
    for k in range(n):
        rows[k // row_length, k % row_length] = vals[k]
    return n
