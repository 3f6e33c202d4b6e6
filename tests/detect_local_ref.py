"""The local floor of the row detector (include/zfft.h, zfft_plan_detect_local) in numpy float32,
a plain loop; the runs, records and occupancy are detect_ref's own code, by import.

With h = half_window, gd = guard, n = row_len:
1. reference cells of column j: the columns c with gd < |c - j| <= gd + h and 0 <= c < n; the
   window is cut at the row's ends (no wrap, no mirror).
2. population: the finite values among them, m_j of them.
3. floor_j = np.sort(w[np.isfinite(w)])[k], k = int(floor(q * float(m_j - 1))); m_j == 0: NaN.
4. thr_j = floor_j + float32(threshold_db), one float32 addition; column j is on when
   v[j] >= thr_j (+inf on; NaN and -inf off; a NaN floor: off).
5. runs, records, found and occupancy as detect_ref.ref_detect (its rules 4-7).
6. floor[i] stays the row-global floor of detect_ref.ref_detect.
"""
import numpy as np

import detect_ref as dr


def window_columns(j, row_len, h, guard):
    """The reference cells of column j, ascending."""
    left = np.arange(j - guard - h, j - guard)
    right = np.arange(j + guard + 1, j + guard + h + 1)
    c = np.concatenate([left, right])
    return c[(c >= 0) & (c < row_len)]


def ref_local_floors(rows, row_len, h, guard, q):
    """float32 (count, n_win): floor_j for j < row_len, NaN at or beyond row_len."""
    rows = np.asarray(rows, dtype=np.float32)
    rows = rows.reshape(-1, rows.shape[-1])
    out = np.full(rows.shape, np.nan, dtype=np.float32)
    for i in range(rows.shape[0]):
        v = rows[i, :row_len]
        for j in range(row_len):
            w = v[window_columns(j, row_len, h, guard)]
            fin = w[np.isfinite(w)]
            if fin.size:
                out[i, j] = np.sort(fin)[int(np.floor(q * float(fin.size - 1)))]
    return out


def fast_local_floors(rows, row_len, h, guard, q):
    """ref_local_floors without the per-column loop, for the wide rows of the GPU tests (pinned
    against the loop by test_detect_local_host.py): the row padded with NaN, the two sides of
    every window as sliding views, one sort per row with the non-finite values (as NaN) last."""
    rows = np.asarray(rows, dtype=np.float32)
    rows = rows.reshape(-1, rows.shape[-1])
    out = np.full(rows.shape, np.nan, dtype=np.float32)
    pad = guard + h
    view = np.lib.stride_tricks.sliding_window_view
    for i in range(rows.shape[0]):
        v = rows[i, :row_len].copy()
        v[~np.isfinite(v)] = np.nan
        p = np.concatenate([np.full(pad, np.nan, np.float32), v, np.full(pad, np.nan, np.float32)])
        # column j is p[pad + j]: its left cells p[j .. j + h), its right cells p[j + pad + guard + 1 ..][:h]
        w = np.concatenate([view(p, h)[:row_len], view(p, h)[pad + guard + 1:pad + guard + 1 + row_len]], axis=1)
        w = np.sort(w, axis=1)  # NaN last
        m = np.count_nonzero(~np.isnan(w), axis=1)
        k = np.floor(q * (m - 1).astype(np.float64)).astype(np.int64)
        got = w[np.arange(row_len), np.maximum(k, 0)]
        got[m == 0] = np.nan
        out[i, :row_len] = got
    return out


def ref_detect_local(rows, row_len, h, guard, quantile=0.5, threshold_db=12.0, min_width=1, K=8, floors=None):
    """(floor, found, events, occ) as detect_ref.ref_detect, the on-flags by the local rule.
    The run code is not copied: ref_detect is given a marker row, 2.0 where the local rule has
    the column on and 0.0 elsewhere, plus one 0.0 column so that its floor at quantile 0 is 0.0
    even on an all-on row; with threshold 1 its on columns, runs, found and occupancy are the
    local rule's.  The peaks are then taken from the real values, as its rule 5 says."""
    rows = np.asarray(rows, dtype=np.float32)
    rows = rows.reshape(-1, rows.shape[-1])
    count, n_win = rows.shape
    if floors is None:
        floors = ref_local_floors(rows, row_len, h, guard, quantile)
    add = np.float32(threshold_db)
    with np.errstate(over="ignore", invalid="ignore"):
        thr = (floors[:, :row_len] + add).astype(np.float32)
        on = rows[:, :row_len] >= thr  # NaN on either side: off
    marker = np.zeros((count, row_len + 1), dtype=np.float32)
    marker[:, :row_len][on] = 2.0
    _, found, mev, mocc = dr.ref_detect(marker, row_len + 1, 0.0, 1.0, min_width, K)
    floor = dr.ref_detect(rows, row_len, quantile, threshold_db, min_width, 1)[0]  # rule 6
    events = np.zeros((count, K), dtype=dr.EMISSION)
    for i in range(count):
        for r in range(min(int(found[i]), K)):
            a, b = int(mev[i, r]["first"]), int(mev[i, r]["last"])
            pk = a + int(np.argmax(rows[i, a:b + 1]))
            events[i, r] = (a, b, pk, rows[i, pk])
    occ = np.zeros(n_win, dtype=np.uint32)
    occ[:row_len] = mocc[:row_len]
    return floor, found, events, occ


def assert_floors_same(got, want, row_len):
    """Floors compared as bits over the row's columns; a zero floor's sign is not defined."""
    g = np.ascontiguousarray(got[:, :row_len]).copy()
    w = np.ascontiguousarray(want[:, :row_len]).copy()
    np.testing.assert_array_equal(np.isnan(g), np.isnan(w))
    g[np.isnan(g)] = 0
    w[np.isnan(w)] = 0
    g[g == 0] = 0.0
    w[w == 0] = 0.0
    np.testing.assert_array_equal(g.view(np.uint32), w.view(np.uint32))


# ---- the "meaning" case: a floor that rises 40 units over the row, +-3 units of noise, tones of
# two columns planted 20 units above it
MEANING_LOCAL = {"seed": 20261, "threshold_db": 12.0, "min_width": 1, "K": 32,
                 "rows": ((512, (20, 130, 300, 470, 505)), (200, (5, 60, 150, 195))),
                 "shapes": ((16, 2, 0.5), (32, 4, 0.75), (8, 2, 0.5)),  # (h, guard, q)
                 "global_runs": {512: 21, 200: 6}, "global_misses": {512: (20, 130), 200: (5, 60)}}


def meaning_row(n, tones):
    rng = np.random.default_rng(MEANING_LOCAL["seed"])
    v = (-150.0 + 40.0 * np.arange(n) / n + rng.uniform(-3.0, 3.0, n)).astype(np.float32)
    for t in tones:
        v[t:t + 2] += np.float32(20.0)
    return v
