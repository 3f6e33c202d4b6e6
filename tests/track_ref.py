"""The emission tracker's rule (include/zfft.h, zfft_plan_track) in plain Python / numpy over the
detector's outputs (found, events): once as a graph over all rows at once (`ref_tracks`: every
link tested, components by union-find) and once as a stream (`RefTracker`: row by row, with the
state a device tracker has to carry), so that the two check each other under any chunking."""
import numpy as np

EMISSION_DTYPE = np.dtype([("first", np.int32), ("last", np.int32), ("peak", np.int32), ("peak_db", np.float32)])
TRACK_DTYPE = np.dtype([("row_first", np.int64), ("row_last", np.int64), ("peak_row", np.int64),
                        ("cells", np.uint64), ("runs", np.uint64), ("col_first", np.int32),
                        ("col_last", np.int32), ("peak_col", np.int32), ("slot_first", np.int32),
                        ("peak_db", np.float32), ("reserved", np.int32)])
assert TRACK_DTYPE.itemsize == 64
STATE_KEYS = ("rows_seen", "open", "unread", "dropped", "short_tracks", "truncated_rows")


def events_array(rows_of_runs, K):
    """(found, events) from a list per row of (first, last[, peak[, peak_db]]) tuples."""
    n = len(rows_of_runs)
    found = np.zeros(n, dtype=np.int32)
    ev = np.zeros((n, K), dtype=EMISSION_DTYPE)
    for t, runs in enumerate(rows_of_runs):
        found[t] = len(runs)
        for s, r in enumerate(runs[:K]):
            first, last = r[0], r[1]
            peak = r[2] if len(r) > 2 else first
            db = r[3] if len(r) > 3 else -50.0
            ev[t, s] = (first, last, peak, db)
    return found, ev


def _used(found, K):
    return min(max(int(found), 0), K)


def linked(a, b, slack):
    return int(a["first"]) <= int(b["last"]) + slack and int(b["first"]) <= int(a["last"]) + slack


class _Agg:
    """A track's record while it grows."""
    __slots__ = ("name", "row_last", "cells", "runs", "col_first", "col_last", "peak_db", "peak_pos")

    def __init__(self, row, slot, e):
        self.name = (row, slot)
        self.row_last = row
        self.cells = int(e["last"]) - int(e["first"]) + 1
        self.runs = 1
        self.col_first, self.col_last = int(e["first"]), int(e["last"])
        self.peak_db = np.float32(e["peak_db"]) + np.float32(0.0)  # -0.0 -> 0.0: a zero maximum is +0.0
        self.peak_pos = (row, int(e["peak"]))

    def merge(self, o):
        self.name = min(self.name, o.name)
        self.row_last = max(self.row_last, o.row_last)
        self.cells += o.cells
        self.runs += o.runs
        self.col_first = min(self.col_first, o.col_first)
        self.col_last = max(self.col_last, o.col_last)
        if o.peak_db > self.peak_db:
            self.peak_db, self.peak_pos = o.peak_db, o.peak_pos
        elif o.peak_db == self.peak_db:
            self.peak_pos = min(self.peak_pos, o.peak_pos)

    def record(self):
        return (self.name[0], self.row_last, self.peak_pos[0], self.cells, self.runs, self.col_first,
                self.col_last, self.peak_pos[1], self.name[1], self.peak_db, 0)


def _records(aggs, key):
    out = np.zeros(len(aggs), dtype=TRACK_DTYPE)
    for i, a in enumerate(sorted(aggs, key=key)):
        out[i] = a.record()
    return out


def _report_key(a):
    return (a.row_last, a.name[0], a.name[1])


def ref_tracks(found, events, gap=0, slack=0, min_rows=1):
    """All rows at once, no flush: (reported in read order, open in open order, state dict)."""
    found = np.asarray(found)
    S, K = events.shape
    nodes = [(t, s) for t in range(S) for s in range(_used(found[t], K))]
    index = {n: i for i, n in enumerate(nodes)}
    parent = list(range(len(nodes)))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for (t, s) in nodes:
        for ta in range(max(0, t - gap - 1), t):
            for sa in range(_used(found[ta], K)):
                if linked(events[ta, sa], events[t, s], slack):
                    ra, rb = find(index[(ta, sa)]), find(index[(t, s)])
                    if ra != rb:
                        parent[max(ra, rb)] = min(ra, rb)
    comps = {}
    for i, (t, s) in enumerate(nodes):
        a = _Agg(t, s, events[t, s])
        r = find(i)
        if r in comps:
            comps[r].merge(a)
        else:
            comps[r] = a
    closed = [a for a in comps.values() if a.row_last + gap + 1 < S]
    opened = [a for a in comps.values() if not a.row_last + gap + 1 < S]
    rep = [a for a in closed if a.row_last - a.name[0] + 1 >= min_rows]
    state = dict(rows_seen=S, open=len(opened), unread=len(rep), dropped=0,
                 short_tracks=len(closed) - len(rep), truncated_rows=int(np.sum(found > K)))
    return _records(rep, _report_key), _records(opened, lambda a: a.name), state


class RefTracker:
    """The rule as a stream: push rows in any cut, read in any interleaving."""

    def __init__(self, K, gap=0, slack=0, min_rows=1, max_tracks=1 << 22):
        self.K, self.gap, self.slack, self.min_rows, self.max_tracks = K, gap, slack, min_rows, max_tracks
        self.reset()

    def reset(self):
        self.S = 0
        self.frontier = []   # [(row, [(record, track id)])] of the last gap + 1 rows
        self.open_tracks = {}  # id -> _Agg
        self.alias = {}      # merged id -> surviving id
        self.next_id = 0
        self.store = []
        self.dropped = self.short = self.truncated = 0

    def _id(self, i):
        while i in self.alias:
            i = self.alias[i]
        return i

    def _close(self, agg):
        if agg.row_last - agg.name[0] + 1 < self.min_rows:
            self.short += 1
        elif len(self.store) >= self.max_tracks:
            self.dropped += 1
        else:
            self.store.append(agg)

    def push(self, found, events):
        found = np.asarray(found)
        events = np.asarray(events).reshape(len(found), self.K)
        for i in range(len(found)):
            t = self.S
            self.truncated += int(found[i] > self.K)
            mine = []
            for s in range(_used(found[i], self.K)):
                e = events[i, s].copy()
                tid = self.next_id
                self.next_id += 1
                self.open_tracks[tid] = _Agg(t, s, e)
                for row, runs in self.frontier:
                    if not 1 <= t - row <= self.gap + 1:
                        continue
                    for ea, ida in runs:
                        if linked(ea, e, self.slack):
                            a, b = self._id(ida), self._id(tid)
                            if a != b:
                                self.open_tracks[a].merge(self.open_tracks.pop(b))
                                self.alias[b] = a
                mine.append((e, tid))
            self.frontier = [(r, runs) for r, runs in self.frontier if t - r <= self.gap] + [(t, mine)]
            self.S += 1
            closing = [k for k, a in self.open_tracks.items() if a.row_last + self.gap + 1 < self.S]
            for a in sorted((self.open_tracks.pop(k) for k in closing), key=_report_key):
                self._close(a)

    def flush(self):
        for a in sorted(self.open_tracks.values(), key=_report_key):
            self._close(a)
        self.open_tracks, self.frontier, self.alias = {}, [], {}

    def read(self, max=None):
        n = len(self.store) if max is None else min(max, len(self.store))
        out, self.store = self.store[:n], self.store[n:]
        return _records(out, lambda a: 0)  # (already in read order; the sort is stable)

    def open(self):
        return _records(list(self.open_tracks.values()), lambda a: a.name)

    def state(self):
        return dict(rows_seen=self.S, open=len(self.open_tracks), unread=len(self.store), dropped=self.dropped,
                    short_tracks=self.short, truncated_rows=self.truncated)


def assert_tracks_same(got, want, what=""):
    """Every field equal, peak_db as bits."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == TRACK_DTYPE and want.dtype == TRACK_DTYPE, (got.dtype, want.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for name in TRACK_DTYPE.names:
        g, w = got[name], want[name]
        if name == "peak_db":
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (what, name, int(bad[0]), got[bad[0]], want[bad[0]])


def scene_rows():
    """The pinned scene: a carrier, a burst, a hopper, a chirp, two arms that merge, a keyed signal."""
    rng = np.random.default_rng(7)
    R, W = 96, 128
    rows = (-120 + 1.5 * rng.standard_normal((R, W))).astype(np.float32)
    rows[:, 10:13] = -80
    rows[20:30, 30:38] = -85
    for k in range(8):
        rows[8 * k + 16:8 * k + 20, 50 + 6 * (k % 3):53 + 6 * (k % 3)] = -82
    for i in range(40):
        rows[30 + i, 80 + i // 2:83 + i // 2] = -84
    for i in range(12):
        rows[60 + i, 100 - i:102 - i] = -83
        rows[60 + i, 110 + i // 3:112 + i // 3] = -83
    for i in range(12, 20):
        rows[60 + i, 88:116] = -83
    rows[40:50:2, 120:124] = -81
    return rows


SCENE_DETECT = dict(row_len=128, quantile=0.5, threshold_db=12.0, min_width=2, K=8)
# (gap, slack, min_rows) -> (reported, open, short_tracks), all 96 rows given and no flush
SCENE_TABLE = {(0, 0, 1): (15, 1, 0), (0, 0, 3): (10, 1, 5), (1, 0, 3): (11, 1, 0), (0, 1, 3): (10, 1, 5),
               (2, 2, 1): (11, 1, 0)}
