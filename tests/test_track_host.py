"""CPU checks of the emission tracker: the rule of include/zfft.h (zfft_plan_track) as
track_ref states it, pinned clause by clause on hand-made records and on the pinned scene; the
reference's own invariance under chunking; the C-ABI's new names; and the form chooser and the
host side of the open table (csrc/zfft_track_plan.cpp) swept by a stand-alone program under
ASan + UBSan."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np

import detect_ref as dr
import track_ref as tr
from test_host import header_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["zfft_plan_track", "zfft_track_shape", "zfft_track_push_device", "zfft_track_push", "zfft_track_read",
         "zfft_track_open", "zfft_track_flush", "zfft_track_state", "zfft_track_reset"]


def _both(rows_of_runs, K=4, gap=0, slack=0, min_rows=1):
    """(reported, open, state) of hand-made rows, the graph form checked against the stream."""
    found, ev = tr.events_array(rows_of_runs, K)
    rep, op, st = tr.ref_tracks(found, ev, gap, slack, min_rows)
    t = tr.RefTracker(K, gap, slack, min_rows)
    t.push(found, ev)
    assert t.state() == st
    tr.assert_tracks_same(t.read(), rep)
    tr.assert_tracks_same(t.open(), op)
    return rep, op, st


def _spans(recs):
    return [(int(r["row_first"]), int(r["row_last"]), int(r["col_first"]), int(r["col_last"]), int(r["runs"]))
            for r in recs]


def test_link_and_no_link_at_slack_0_and_1():
    e = []  # an empty row closes everything at gap 0
    share = [[(10, 12)], [(12, 15)], e]          # share column 12
    touch = [[(10, 12)], [(13, 15)], e]          # merely touch
    apart = [[(10, 12)], [(14, 15)], e]          # one column between
    assert _spans(_both(share, slack=0)[0]) == [(0, 1, 10, 15, 2)]
    assert _spans(_both(touch, slack=0)[0]) == [(0, 0, 10, 12, 1), (1, 1, 13, 15, 1)]
    assert _spans(_both(touch, slack=1)[0]) == [(0, 1, 10, 15, 2)]
    assert _spans(_both(apart, slack=1)[0]) == [(0, 0, 10, 12, 1), (1, 1, 14, 15, 1)]
    assert _spans(_both(apart, slack=2)[0]) == [(0, 1, 10, 15, 2)]
    # the rule is symmetric: the later run may lie below the earlier one
    assert _spans(_both([[(13, 15)], [(10, 12)], e], slack=1)[0]) == [(0, 1, 10, 15, 2)]
    # runs of one row are never linked to each other, however close
    assert _spans(_both([[(10, 12), (13, 15)], e], slack=64)[0]) == [(0, 0, 10, 12, 1), (0, 0, 13, 15, 1)]


def test_gap_0_1_7_across_absent_rows():
    e = []
    for gap in (0, 1, 7):
        for absent in range(0, 10):
            rows = [[(5, 6)]] + [e] * absent + [[(5, 6)]] + [e] * 9
            rep = _both(rows, gap=gap)[0]
            if absent <= gap:
                assert _spans(rep) == [(0, absent + 1, 5, 6, 2)], (gap, absent)
            else:
                assert _spans(rep) == [(0, 0, 5, 6, 1), (absent + 1, absent + 1, 5, 6, 1)], (gap, absent)
    # the rows in between do not matter: a row with an unrelated run is as good as an empty one
    rows = [[(5, 6)], [(40, 41)], [(5, 6)], e, e]
    assert _spans(_both(rows, gap=1)[0]) == [(1, 1, 40, 41, 1), (0, 2, 5, 6, 2)]


def test_a_y_merge_and_a_split():
    e = []
    merge = [[(10, 11), (20, 21)], [(11, 12), (19, 20)], [(12, 19)], e]
    rep = _both(merge)[0]
    assert _spans(rep) == [(0, 2, 10, 21, 5)] and int(rep[0]["cells"]) == 2 * 4 + 8 and int(rep[0]["slot_first"]) == 0
    split = [[(12, 19)], [(11, 12), (19, 20)], [(10, 11), (20, 21)], e]
    assert _spans(_both(split)[0]) == [(0, 2, 10, 21, 5)]
    # two tracks side by side that never meet stay two, in (row_last, row_first, slot_first) order
    side = [[(10, 11), (20, 21)], [(10, 11), (20, 21)], [(20, 21)], e]
    assert _spans(_both(side)[0]) == [(0, 1, 10, 11, 2), (0, 2, 20, 21, 3)]


def test_the_peak_tie_break():
    e = []
    # equal peak_db in two rows: the lower row; a higher value anywhere wins over both
    rows = [[(5, 9, 7, -40.0)], [(5, 9, 6, -30.0)], [(5, 9, 5, -30.0)], e]
    r = _both(rows)[0][0]
    assert (int(r["peak_row"]), int(r["peak_col"]), float(r["peak_db"])) == (1, 6, -30.0)
    # equal peak_db in two runs of one row (a merge): the lower column
    rows = [[(5, 9, 9, -30.0), (20, 24, 20, -30.0)], [(9, 20, 12, -35.0)], e]
    r = _both(rows)[0][0]
    assert (int(r["peak_row"]), int(r["peak_col"]), int(r["runs"])) == (0, 9, 3)
    # lexicographic: the lower row wins with the higher column
    rows = [[(5, 9, 9, -30.0)], [(5, 9, 5, -30.0)], e]
    r = _both(rows)[0][0]
    assert (int(r["peak_row"]), int(r["peak_col"])) == (0, 9)
    # a float comparison: -0.0 and 0.0 are equal (the lower (row, peak) holds), reported as 0.0
    for a, b in ((-0.0, 0.0), (0.0, -0.0)):
        r = _both([[(5, 9, 8, a)], [(5, 9, 6, b)], e])[0][0]
        assert (int(r["peak_row"]), int(r["peak_col"])) == (0, 8)
        assert r["peak_db"] == 0.0 and not np.signbit(r["peak_db"])
    # +inf is a value like any other
    r = _both([[(5, 9, 8, -3.0)], [(5, 9, 6, np.inf)], e])[0][0]
    assert (int(r["peak_row"]), int(r["peak_col"]), float(r["peak_db"])) == (1, 6, np.inf)


def test_slot_first_names_a_track():
    e = []
    rows = [[(1, 2), (10, 11), (20, 21)], [(10, 11), (20, 21)], e]
    rep = _both(rows)[0]
    assert [(int(r["row_first"]), int(r["slot_first"])) for r in rep] == [(0, 0), (0, 1), (0, 2)]
    # the lowest slot among its runs in row_first, not its first link
    rows = [[(1, 2)], [(30, 31), (40, 41)], [(31, 40)], e]
    rep = _both(rows)[0]
    assert [(int(r["row_first"]), int(r["slot_first"]), int(r["runs"])) for r in rep] == [(0, 0, 1), (1, 0, 3)]


def test_min_rows_and_short_tracks():
    e = []
    rows = [[(1, 2), (10, 11)], [(10, 11)], [(10, 11), (30, 31)], [(30, 31)], e]
    for min_rows, want, short in ((1, 3, 0), (2, 2, 1), (3, 1, 2), (4, 0, 3)):
        rep, _, st = _both(rows, min_rows=min_rows)
        assert len(rep) == want and st["short_tracks"] == short and st["unread"] == want, min_rows


def test_closing_exactly_when_no_later_row_can_reach():
    for gap in (0, 1, 7):
        found, ev = tr.events_array([[(5, 6)]] + [[]] * 10, 4)
        t = tr.RefTracker(4, gap)
        for S in range(1, 11):
            t.push(found[S - 1:S], ev[S - 1:S])
            st = t.state()
            closed = 0 + gap + 1 < S  # row_last = 0
            assert (st["open"], st["unread"]) == ((0, 1) if closed else (1, 0)), (gap, S)
            assert tr.ref_tracks(found[:S], ev[:S], gap)[2]["unread"] == int(closed)
        # not one row sooner: a run in row gap + 1 still links
        rows = [[(5, 6)]] + [[]] * gap + [[(5, 6)]] + [[]] * 9
        assert _spans(_both(rows, gap=gap)[0]) == [(0, gap + 1, 5, 6, 2)]


def test_flush():
    found, ev = tr.events_array([[(5, 6), (20, 21)], [(5, 6)], [(5, 6)]], 4)
    t = tr.RefTracker(4, gap=2, min_rows=2)
    t.push(found, ev)
    assert t.state()["open"] == 2 and t.state()["unread"] == 0
    t.flush()
    st = t.state()
    assert (st["open"], st["unread"], st["short_tracks"], st["rows_seen"]) == (0, 1, 1, 3)
    assert _spans(t.read()) == [(0, 2, 5, 6, 3)]
    # the row counter went on, and later rows link to nothing earlier
    t.push(found[1:2], ev[1:2])
    t.push(*tr.events_array([[], [], []], 4))
    assert _spans(t.read()) == [] and t.state()["short_tracks"] == 2 and t.state()["rows_seen"] == 7
    # among themselves the flushed tracks keep the read order
    t = tr.RefTracker(4, gap=3)
    t.push(*tr.events_array([[(1, 2), (10, 11), (20, 21)], [(10, 11)], [(1, 2)]], 4))
    t.flush()
    assert [(int(r["row_last"]), int(r["slot_first"])) for r in t.read()] == [(0, 2), (1, 1), (2, 0)]


def test_truncated_rows_and_clamping_of_found():
    K = 2
    found, ev = tr.events_array([[(1, 2), (10, 11), (20, 21)], [(1, 2), (10, 11), (20, 21)], []], K)
    assert found.tolist() == [3, 3, 0]
    rep, _, st = tr.ref_tracks(found, ev)
    assert st["truncated_rows"] == 2 and _spans(rep) == [(0, 1, 1, 2, 2), (0, 1, 10, 11, 2)]
    # found < 0 is 0, found > K is K: the records beyond are never looked at
    ev[2] = [(1, 2, 1, -50.0), (10, 11, 10, -50.0)]
    for f2, runs in ((-1, 2), (-2**31, 2), (0, 2), (1, 3), (2, 3), (2**31 - 1, 3)):
        found[2] = f2
        t = tr.RefTracker(K)
        t.push(found, ev)
        t.flush()
        rep = t.read()
        assert int(rep["runs"].max()) == runs and t.state()["truncated_rows"] == 2 + (f2 > K), f2
        tr.assert_tracks_same(np.sort(rep, order=["row_last", "row_first", "slot_first"]), rep)


def test_a_full_store_drops_and_counts():
    found, ev = tr.events_array([[(i, i)] if i % 2 == 0 else [] for i in range(20)], 4)
    t = tr.RefTracker(4, max_tracks=4)
    t.push(found, ev)
    st = t.state()
    assert (st["unread"], st["dropped"], st["open"]) == (4, 6, 0) and len(t.read()) == 4


@functools.lru_cache(maxsize=None)
def _scene():
    rows = tr.scene_rows()
    _, found, ev, _ = dr.ref_detect(rows, **tr.SCENE_DETECT)
    assert found.max() <= 5
    found.setflags(write=False)
    ev.setflags(write=False)
    return found, ev


def test_the_pinned_scene():
    found, ev = _scene()
    for (gap, slack, min_rows), (n_rep, n_open, n_short) in tr.SCENE_TABLE.items():
        rep, op, st = tr.ref_tracks(found, ev, gap, slack, min_rows)
        assert (len(rep), len(op), st["short_tracks"]) == (n_rep, n_open, n_short), (gap, slack, min_rows)
        assert st["truncated_rows"] == 0 and st["dropped"] == 0 and st["rows_seen"] == 96
    rep, op, _ = tr.ref_tracks(found, ev, 1, 0, 3)
    last = rep[-1]
    assert (int(last["row_first"]), int(last["row_last"]), int(last["slot_first"])) == (30, 79, 1)
    assert (int(last["col_first"]), int(last["col_last"])) == (80, 115)
    assert (float(last["peak_db"]), int(last["peak_row"]), int(last["peak_col"])) == (-83.0, 60, 100)
    assert (int(last["runs"]), int(last["cells"])) == (68, 388)
    keyed = [r for r in rep if r["col_first"] >= 120]
    assert len(keyed) == 1 and _spans(keyed) == [(40, 48, 120, 123, 5)] and int(keyed[0]["cells"]) == 20
    keyed0 = [r for r in tr.ref_tracks(found, ev, 0, 0, 1)[0] if r["col_first"] >= 120]
    assert [int(r["row_last"] - r["row_first"]) for r in keyed0] == [0] * 5  # at gap 0: five short ones
    assert _spans(op) == [(0, 95, 10, 12, 96)] and int(op[0]["cells"]) == 288


def test_chunking_invariance_of_the_reference():
    """The sequence of reads and the final open tracks and state do not depend on how the rows
    are cut into pushes nor on where the reads fall between them."""
    found, ev = _scene()
    rng = np.random.default_rng(11)
    for (gap, slack, min_rows) in tr.SCENE_TABLE:
        rep, op, st = tr.ref_tracks(found, ev, gap, slack, min_rows)
        cuts = [[96], [1] * 96, [7, 1, 40, 48]] + [rng.multinomial(96, np.ones(9) / 9).tolist() for _ in range(3)]
        for cut in cuts:
            for read_every_push in (False, True):
                t = tr.RefTracker(8, gap, slack, min_rows)
                got, at = [], 0
                for n in cut:
                    if n:
                        t.push(found[at:at + n], ev[at:at + n])
                    at += n
                    if read_every_push:
                        got.append(t.read(3))
                got.append(t.read())
                st2 = t.state()
                assert st2["unread"] == 0 and {**st2, "unread": st["unread"]} == st
                tr.assert_tracks_same(np.concatenate(got), rep, (gap, slack, min_rows, cut))
                tr.assert_tracks_same(t.open(), op)
                # every prefix too: the closed set after S rows is {row_last <= S - gap - 2}
        for S in (1, gap + 2, 40, 77):
            part = tr.ref_tracks(found[:S], ev[:S], gap, slack, min_rows)[0]
            assert np.all(part["row_last"] <= S - gap - 2)
            tr.assert_tracks_same(part, rep[rep["row_last"] <= S - gap - 2])


def test_new_names_are_declared_and_exported(zfft_lib):
    from pypanadapter_amd import _lib
    from pypanadapter_amd.engine import TRACK_DTYPE
    declared = header_functions()
    for name in NAMES:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert getattr(zfft_lib, name).argtypes is not None, name
    assert TRACK_DTYPE == tr.TRACK_DTYPE and TRACK_DTYPE.itemsize == 64
    text = open(os.path.join(ROOT, "include", "zfft.h")).read()
    body = text[text.index("typedef struct zfft_track {"):text.index("} zfft_track;")]
    order = [body.index(f) for f in ("int64_t row_first, row_last;", "int64_t peak_row;", "uint64_t cells;",
                                     "uint64_t runs;", "int32_t col_first, col_last;", "int32_t peak_col;",
                                     "int32_t slot_first;", "float peak_db;", "int32_t reserved;")]
    assert order == sorted(order)  # the header's fields in TRACK_DTYPE's order


def track_form(lib, K, gap, count):
    """(chunk_rows, pass_rows, passes, chunks) of zfft__track_form, or None where it refuses."""
    hook = lib.zfft__track_form
    hook.argtypes = [ctypes.c_int32] * 3 + [ctypes.POINTER(ctypes.c_int32)]
    hook.restype = ctypes.c_int
    out = (ctypes.c_int32 * 4)()
    return None if hook(K, gap, count, out) else tuple(out)


def test_form_chooser_through_the_hook(zfft_lib):
    assert track_form(zfft_lib, 8, 0, 69632) == (64, 131008, 1, 1088)   # cfg2's step: one pass
    assert track_form(zfft_lib, 32, 7, 2048)[0] == 16 and track_form(zfft_lib, 32, 7, 2048)[2] == 1
    assert track_form(zfft_lib, 8, 7, 1)[::3] == (16, 1)
    assert track_form(zfft_lib, 32, 0, 1 << 26)[2] == -(-(1 << 26) // track_form(zfft_lib, 32, 0, 1 << 26)[1])
    for K in (1, 8, 32):
        for gap in (0, 7):
            for count in (1, 15, 16, 17, 8191, 8192, 16383, 16384, 69632, 1 << 26):
                c, p, n, ch = track_form(zfft_lib, K, gap, count)
                assert c in (16, 32, 64) and c * K <= 2048 and p % c == 0 and (p + gap + 1) * K <= 1 << 20
                assert (n - 1) * p < count <= n * p and ch == -(-min(count, p) // c)
    for bad in ((0, 0, 1), (33, 0, 1), (8, -1, 1), (8, 8, 1), (8, 0, 0), (8, 0, (1 << 26) + 1)):
        assert track_form(zfft_lib, *bad) is None, bad


def test_track_form_sweep_sanitized(tmp_path):
    """The chooser over its domain and the open table's host side as a stand-alone g++ program (no
    HIP, no Python in the child) under AddressSanitizer + UBSan: tests/host/track_form_sweep.cpp."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/host/track_form_sweep.cpp"
    csrc = os.path.join(ROOT, "pypanadapter_amd", "csrc")
    exe = str(tmp_path / "track_form_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", csrc, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "track_form_sweep.cpp"),
                    os.path.join(csrc, "zfft_track_plan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "track_form_sweep: ok" in r.stdout, r.stdout
