"""GPU checks of the emission tracker (zfft_plan_track: the detector's runs linked across rows
into tracks, on the device) against track_ref, the rule of include/zfft.h in plain Python (pinned
on the CPU by test_track_host.py), on the very (found, events) given to the device.  The rule is
integers and one float maximum: every field compares exactly (peak_db as bits), so there is no
tolerance to choose.  Inputs keep dropped == 0 and truncated_rows == 0 unless the test is about
them; the device chain's rows are test_gpu_detect.py's device case, two of which hold more than K
runs -- the rule defines that too, and the reference follows it."""
import ctypes
import functools

import numpy as np
import pytest

import detect_ref as dr
import stall
import track_ref as tr
import welch_average_ref as war

pytestmark = pytest.mark.gpu
FS = war.FS


@pytest.fixture(scope="module", autouse=True)
def _gpu(zfft_lib):
    from pypanadapter_amd import device_count
    assert device_count() >= 1, "GPU tests need a HIP device"


def _form(plan, count):
    """(chunk_rows, pass_rows, passes, chunks) of a push of `count` rows (hook zfft__plan_track_form)."""
    hook = plan.lib.zfft__plan_track_form
    hook.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]
    hook.restype = ctypes.c_int
    out = (ctypes.c_int32 * 4)()
    assert hook(plan._plan, count, out) == 0
    return tuple(out)


def _plan(K, W=64):
    """A plan whose detector has max_per_row = K: the tracker only takes K from it."""
    from pypanadapter_amd import ZoomFFT
    plan = ZoomFFT(max(W, 32), 1, FS, n_win=W)
    plan.set_detect(0.5, 12.0, 1, K)
    return plan


def _push_cut(plan, found, ev, cut):
    at = 0
    for n in cut:
        plan.track_push(found[at:at + n], ev[at:at + n])
        at += n
    assert at == len(found)


def _check_whole(plan, found, ev, params, cuts, what=""):
    """For every cut: set_track(params), the pushes, then tracks() / open_tracks() / track_state()
    against ref_tracks of all the rows."""
    rep, op, st = tr.ref_tracks(found, ev, *params)
    for cut in cuts:
        plan.set_track(*params)
        _push_cut(plan, found, ev, cut)
        assert plan.track_state() == st, (what, params, cut)
        tr.assert_tracks_same(plan.open_tracks(), op, (what, params, cut, "open"))
        tr.assert_tracks_same(plan.tracks(), rep, (what, params, cut))
        assert plan.track_state() == {**st, "unread": 0}
    return rep, op, st


# ---------------------------------------------------------------- 1. the pinned scene
@functools.lru_cache(maxsize=None)
def _scene():
    rows = tr.scene_rows()
    rows.setflags(write=False)
    return rows, dr.ref_detect(rows, **tr.SCENE_DETECT)


@pytest.mark.parametrize("params", list(tr.SCENE_TABLE), ids=lambda p: "gap%d_slack%d_min%d" % p)
def test_scene_through_detect_in_three_cuts(params):
    from pypanadapter_amd import ZoomFFT
    rows, want = _scene()
    d = tr.SCENE_DETECT
    with ZoomFFT(128, 1, FS, n_win=128) as plan:
        plan.set_detect(d["quantile"], d["threshold_db"], d["min_width"], d["K"])
        _, found, ev = plan.detect(rows)
        dr.assert_same((want[0], found, ev), want[:3])
        rep, op, st = _check_whole(plan, found, ev, params, ([96], [1] * 96, [7, 1, 40, 48]), "scene")
        assert (len(rep), len(op), st["short_tracks"]) == tr.SCENE_TABLE[params]
        assert st["dropped"] == 0 and st["truncated_rows"] == 0 and plan.track_shape() == (*params, 65536)


# ---------------------------------------------------------------- 2. partial reads
@pytest.mark.parametrize("cut", [[96], [1] * 96, [7, 1, 40, 48], [30, 30, 36]], ids=["whole", "rows", "cut4", "cut3"])
def test_partial_reads_interleaved_with_pushes(cut):
    rows, want = _scene()
    found, ev = want[1], want[2]
    rep = tr.ref_tracks(found, ev, 0, 0, 1)[0]
    with _plan(8, 128) as plan:
        plan.set_track(0, 0, 1)
        ref = tr.RefTracker(8, 0, 0, 1)
        got, at = [], 0
        for n in cut:
            plan.track_push(found[at:at + n], ev[at:at + n])
            ref.push(found[at:at + n], ev[at:at + n])
            at += n
            part = plan.tracks(max=3)
            tr.assert_tracks_same(part, ref.read(3), (cut, at))
            got.append(part)
            assert plan.track_state() == ref.state()
        while plan.track_state()["unread"]:
            got.append(plan.tracks(max=3))
            assert 1 <= len(got[-1]) <= 3
        assert len(plan.tracks(max=3)) == 0
        tr.assert_tracks_same(np.concatenate(got), rep, cut)


# ---------------------------------------------------------------- 3. K = 1 and K = 32
@pytest.mark.parametrize("wide_first", [False, True])
def test_k32_one_run_across_thirty_two(wide_first):
    comb = [(4 * i, 4 * i + 1, 4 * i + (i % 2), -60.0 - i) for i in range(32)]
    wide = [(0, 127, 77, -70.0)]
    found, ev = tr.events_array([wide, comb] if wide_first else [comb, wide], 32)
    with _plan(32, 128) as plan:
        for gap in (0, 7):
            plan.set_track(gap, 0, 1)
            plan.track_push(found, ev)
            op = plan.open_tracks()
            tr.assert_tracks_same(op, tr.ref_tracks(found, ev, gap)[1])
            assert len(op) == 1 and int(op[0]["runs"]) == 33 and int(op[0]["cells"]) == 64 + 128
            assert (int(op[0]["peak_row"]), int(op[0]["peak_col"]), float(op[0]["peak_db"])) == (int(wide_first), 0, -60.0)
            plan.track_flush()
            tr.assert_tracks_same(plan.tracks(), op)


def test_k1_chains_and_breaks():
    rng = np.random.default_rng(3)
    runs, c = [], 30
    for r in range(150):
        c = int(np.clip(c + rng.integers(-3, 4), 2, 60))
        runs.append([] if rng.random() < 0.2 else [(c, c + 1, c + int(rng.integers(0, 2)), float(-60 - rng.integers(0, 3)))])
    found, ev = tr.events_array(runs, 1)
    with _plan(1) as plan:
        for params in ((0, 0, 1), (1, 1, 2), (7, 0, 1)):
            rep = _check_whole(plan, found, ev, params, ([150], [1] * 150, [16, 17, 117]), "k1")[0]
            assert len(rep) >= 2


# ---------------------------------------------------------------- 4. a serpentine
@pytest.mark.parametrize("K", [16, 32])
def test_serpentine_is_one_track(K):
    """16 bars two columns wide over 64 rows, neighbours joined alternately in row 0 and row 63:
    one component that label propagation has to carry up and down every bar, across every seam."""
    bars = [(4 * b, 4 * b + 1) for b in range(16)]
    top = [(4 * b, 4 * b + 5) for b in range(0, 16, 2)]                        # bars (0,1), (2,3), ...
    bottom = [bars[0]] + [(4 * b, 4 * b + 5) for b in range(1, 15, 2)] + [bars[15]]  # bars (1,2), (3,4), ...
    rows = [top] + [bars] * 62 + [bottom]
    found, ev = tr.events_array(rows, K)
    with _plan(K) as plan:
        plan.set_track(0, 0, 1)
        assert _form(plan, 64)[3] == 4  # four chunks: three seams
        rep, op, st = _check_whole(plan, found, ev, (0, 0, 1), ([64], [31, 33], [1] * 64), "serpentine")
        assert len(rep) == 0 and len(op) == 1 and int(op[0]["runs"]) == 8 + 62 * 16 + 9
        assert (int(op[0]["col_first"]), int(op[0]["col_last"]), int(op[0]["slot_first"])) == (0, 61, 0)
        # without the joins of row 63 the bars pair up: eight tracks
        found2, ev2 = tr.events_array([top] + [bars] * 63, K)
        assert len(_check_whole(plan, found2, ev2, (0, 0, 1), ([64],), "pairs")[1]) == 8


# ---------------------------------------------------------------- 5. seams
def _seam_rows(R, C, gap):
    """64-column rows of hand-made runs: a steady carrier at columns 2-3; a second at 5-6 that is
    absent for exactly `gap` rows across every seam (and for gap + 1 rows across every other);
    a one-row blip in every row, stepping through gap + 2 places four columns apart (never
    linked); and at every seam s = k C, for every d in [-(gap + 1), gap + 1], a one-column track
    of three rows that begins in row s + d (so begins and ends fall on the seam rows and within
    gap of them), each d in a column of its own."""
    rows = [[] for _ in range(R)]
    G = gap + 1
    for r in range(R):
        rows[r].append((2, 3, 2 + r % 2, -50.0 - (r % 7)))
        rows[r].append((8 + 4 * (r % (gap + 2)), 9 + 4 * (r % (gap + 2)), 8 + 4 * (r % (gap + 2)), -61.0))
    absent = set()
    for k in range(1, R // C + 2):
        s = k * C
        n = gap + (k % 2 == 0)
        absent.update(range(s - n // 2, s - n // 2 + n))
        for d in range(-G, G + 1):
            for r in range(s + d, s + d + 3):
                if 0 <= r < R:
                    rows[r].append((46 + d + G, 46 + d + G, 46 + d + G, -55.0 + d))
    for r in range(R):
        if r not in absent:
            rows[r].append((5, 6, 5, -52.0))
    return [sorted(x) for x in rows]


@pytest.mark.parametrize("gap", [0, 2, 7])
def test_seams(gap):
    K = 32
    with _plan(K) as plan:
        plan.set_track(gap, 0, 1)
        C = _form(plan, 100)[0]
        assert C == 16 and _form(plan, 3 * C + 1)[3] == 4 and _form(plan, C - 1)[3] == 1
        for R in (3 * C + 1, C - 1, gap + 1):
            found, ev = tr.events_array(_seam_rows(R, C, gap), K)
            assert found.max() <= K
            cuts = [[R]]
            if R > 2 * C:
                for s in (C, 2 * C):
                    cuts += [[s - 1, R - s + 1], [s, R - s], [s + 1, R - s - 1], [s - 1, 1, 1, R - s - 1]]
            elif R > 2:
                cuts += [[1, R - 1], [R - 1, 1], [1] * R]
            rep, op, st = _check_whole(plan, found, ev, (gap, 0, 1), cuts, f"seams R={R}")
            assert st["open"] >= 2
            if R > 2 * C:
                assert len(rep) > R  # the blips alone are one a row


@functools.lru_cache(maxsize=None)
def _long_call():
    """64 * 256 + 1 rows: chunks of 64 rows (from 64 * 256 rows on) and a last chunk of one row;
    the seam content at K = 4."""
    R, C, gap = 64 * 256 + 1, 64, 1
    rows = [[x for x in r if x[0] < 46 or x[0] == 46 + 2] for r in _seam_rows(R, C, gap)]
    found, ev = tr.events_array(rows, 4)
    ref = tr.RefTracker(4, gap, 0, 2)
    ref.push(found, ev)
    return found, ev, ref.state(), ref.open(), ref.read()


def test_sixty_four_row_chunks():
    found, ev, st, op, rep = _long_call()
    with _plan(4) as plan:
        plan.set_track(1, 0, 2)
        assert _form(plan, len(found))[:3:2] == (64, 1) and _form(plan, 64 * 256 - 1)[0] == 32
        plan.track_push(found, ev)
        assert plan.track_state() == st and st["short_tracks"] > 16000 and st["unread"] > 250
        tr.assert_tracks_same(plan.open_tracks(), op)
        tr.assert_tracks_same(plan.tracks(), rep)


# ---------------------------------------------------------------- 6. pushes shorter than the frontier
def test_one_row_per_call_at_gap_7():
    e = []
    rows = [[(5, 6, 5, -40.0), (20, 21)]] + [e] * 7 + [[(6, 7, 7, -40.0)]] + [e] * 8 + [[(5, 6)]] + [e] * 9
    found, ev = tr.events_array(rows, 4)
    with _plan(4) as plan:
        rep = _check_whole(plan, found, ev, (7, 0, 1), ([1] * len(rows), [len(rows)], [3] * 9), "gap7")[0]
        spans = [(int(r["row_first"]), int(r["row_last"]), int(r["runs"])) for r in rep]
        assert spans == [(0, 0, 1), (0, 8, 2), (17, 17, 1)]  # absent for 7 rows: one track; for 8: two
        assert (int(rep[1]["peak_row"]), int(rep[1]["peak_col"])) == (0, 5)
        # and the state after every single row
        plan.set_track(7, 0, 1)
        ref = tr.RefTracker(4, 7, 0, 1)
        for r in range(len(rows)):
            plan.track_push(found[r:r + 1], ev[r:r + 1])
            ref.push(found[r:r + 1], ev[r:r + 1])
            assert plan.track_state() == ref.state(), r
            tr.assert_tracks_same(plan.open_tracks(), ref.open(), r)


# ---------------------------------------------------------------- 7. truncated rows
def test_truncated_rows():
    from pypanadapter_amd import ZoomFFT
    rows = np.full((6, 64), -120.0, dtype=np.float32)
    rows += np.float32(0.25) * np.arange(64, dtype=np.float32)[None, :] / 64
    for c in (4, 14, 24, 34, 44):
        rows[:5, c:c + 3] = -60.0
    with ZoomFFT(64, 1, FS, n_win=64) as plan:
        plan.set_detect(0.5, 12.0, 1, 2)
        _, found, ev = plan.detect(rows)
        assert found.tolist() == [5] * 5 + [0]
        rep, op, st = _check_whole(plan, found, ev, (0, 0, 1), ([6], [1] * 6), "truncated")
        assert st["truncated_rows"] == 5 and len(rep) == 2 and [int(r["col_first"]) for r in rep] == [4, 14]


# ---------------------------------------------------------------- 8. a full store
def test_full_store_drops_and_counts():
    rows = [[(3 * i, 3 * i + 1)] if i % 2 == 0 else [] for i in range(20)]
    found, ev = tr.events_array(rows, 4)
    want = tr.ref_tracks(found, ev)[0]
    assert len(want) == 10
    with _plan(4) as plan:
        for cut in ([20], [1] * 20, [9, 11]):
            plan.set_track(0, 0, 1, max_tracks=4)
            _push_cut(plan, found, ev, cut)
            st = plan.track_state()
            assert (st["unread"], st["dropped"], st["open"]) == (4, 6, 0), cut
            got = plan.tracks()
            assert len(got) == 4 and len(set(got["row_first"].tolist())) == 4
            for g in got:
                assert any(g.tobytes() == w.tobytes() for w in want), g
            assert plan.track_state()["dropped"] == 6
        # a read makes room again; the ring wraps
        plan.set_track(0, 0, 1, max_tracks=4)
        got = []
        for r in range(20):
            plan.track_push(found[r:r + 1], ev[r:r + 1])
            got.append(plan.tracks(max=1))
        tr.assert_tracks_same(np.concatenate(got), want)
        assert plan.track_state()["dropped"] == 0
        plan.track_reset()
        assert plan.track_state() == dict(rows_seen=0, open=0, unread=0, dropped=0, short_tracks=0, truncated_rows=0)
        plan.set_track(0, 0, 1, max_tracks=16)
        plan.track_push(found, ev)
        tr.assert_tracks_same(plan.tracks(), want)


# ---------------------------------------------------------------- 9. calls and errors
def test_calls_and_errors():
    from pypanadapter_amd import ZoomFFT, _lib
    from pypanadapter_amd.engine import TRACK_DTYPE
    found, ev = tr.events_array([[(5, 6), (20, 21)], [(5, 6)], [(5, 6)]], 4)
    with ZoomFFT(64, 1, FS, n_win=64) as plan:
        lib, P = plan.lib, plan._plan
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        out, n, stats = np.zeros(4, TRACK_DTYPE), ctypes.c_int32(-1), (ctypes.c_uint64 * 6)()
        shape = [ctypes.c_int32(-1) for _ in range(4)]

        def every_call():
            return [lib.zfft_track_push(P, ptr(found), ptr(ev), 3),
                    lib.zfft_track_push_device(P, ctypes.c_void_p(16), ctypes.c_void_p(16), 1, None),
                    lib.zfft_track_read(P, ptr(out), 4, ctypes.byref(n)),
                    lib.zfft_track_open(P, ptr(out), 4, ctypes.byref(n)),
                    lib.zfft_track_flush(P), lib.zfft_track_state(P, ctypes.cast(stats, ctypes.c_void_p)),
                    lib.zfft_track_reset(P), lib.zfft_track_shape(P, *[ctypes.byref(v) for v in shape])]

        assert every_call() == [_lib.ZFFT_EINVAL] * 8 and shape[3].value == 0  # off by default
        with pytest.raises(ValueError):
            plan.set_track(0, 0, 1)  # detection is off
        plan.set_detect(0.5, 12.0, 1, 4)
        assert every_call() == [_lib.ZFFT_EINVAL] * 8  # detection alone enables nothing
        for bad in ((-1, 0, 1, 16), (8, 0, 1, 16), (0, -1, 1, 16), (0, 65, 1, 16), (0, 0, 0, 16), (0, 0, 1, -1),
                    (0, 0, 1, (1 << 22) + 1)):
            with pytest.raises(ValueError):
                plan.set_track(*bad)
        assert every_call() == [_lib.ZFFT_EINVAL] * 8  # a refused setting enables nothing
        plan.set_track(7, 64, 1, 1 << 22)  # the ends of every range
        assert plan.track_shape() == (7, 64, 1, 1 << 22)
        plan.set_track(2, 0, 2, 16)
        assert plan.track_shape() == (2, 0, 2, 16)
        for bad_count in (0, -1, (1 << 26) + 1):
            assert lib.zfft_track_push(P, ptr(found), ptr(ev), bad_count) == _lib.ZFFT_EINVAL
            assert lib.zfft_track_push_device(P, ptr(found), ptr(ev), bad_count, None) == _lib.ZFFT_EINVAL
        assert lib.zfft_track_push(P, None, ptr(ev), 3) == _lib.ZFFT_EINVAL
        assert lib.zfft_track_read(P, ptr(out), -1, ctypes.byref(n)) == _lib.ZFFT_EINVAL
        # host records that break the contract, in a slot the tracker will use
        for slot, rec in (((0, 1), (4, 21, 4, -50.0)),     # not disjoint from (5, 6)
                          ((0, 1), (6, 21, 6, -50.0)),     # shares a column with it
                          ((0, 0), (5, 6, 7, -50.0)),      # peak outside the run
                          ((0, 0), (6, 5, 6, -50.0)),      # last below first
                          ((0, 0), (-1, 6, 0, -50.0)),     # a negative column
                          ((1, 0), (5, 6, 5, np.nan))):    # NaN
            bad = ev.copy()
            bad[slot] = rec
            with pytest.raises(ValueError):
                plan.track_push(found, bad)
        bad = ev.copy()
        bad[1, 1] = (6, 5, 9, np.nan)  # beyond found: never looked at
        plan.track_push(found, bad)
        assert plan.track_state() == dict(rows_seen=3, open=2, unread=0, dropped=0, short_tracks=0, truncated_rows=0)
        plan.track_flush()  # (5, 6) over three rows is reported; (20, 21) is short of min_rows = 2
        st = plan.track_state()
        assert (st["rows_seen"], st["open"], st["unread"], st["short_tracks"]) == (3, 0, 1, 1)
        assert len(plan.open_tracks()) == 0
        plan.track_push(found[1:], ev[1:])  # links to nothing earlier
        plan.track_flush()
        got = plan.tracks()
        assert [(int(t["row_first"]), int(t["row_last"]), int(t["runs"])) for t in got] == [(0, 2, 3), (3, 4, 2)]
        plan.track_push(found, ev)
        plan.track_reset()
        assert plan.track_state() == dict(rows_seen=0, open=0, unread=0, dropped=0, short_tracks=0, truncated_rows=0)
        # set_detect with the same K keeps the tracker, another K resets it
        plan.track_push(found, ev)
        plan.set_detect(0.25, 10.0, 2, 4)
        assert plan.track_state()["rows_seen"] == 3 and len(plan.open_tracks()) == 2
        plan.set_detect(0.5, 12.0, 1, 8)
        assert plan.track_state() == dict(rows_seen=0, open=0, unread=0, dropped=0, short_tracks=0, truncated_rows=0)
        assert plan.track_shape() == (2, 0, 2, 16) and len(plan.open_tracks()) == 0
        f8, e8 = tr.events_array([[(5, 6), (20, 21)], [(5, 6)], [(5, 6)]], 8)
        plan.track_push(f8, e8)
        tr.assert_tracks_same(plan.open_tracks(), tr.ref_tracks(f8, e8, 2, 0, 2)[1])
        plan.set_track(max_tracks=0)  # off
        assert every_call() == [_lib.ZFFT_EINVAL] * 8
        plan.set_track(2, 0, 2, 16)
        plan.set_detect(max_per_row=0)  # detection off switches tracking off
        assert every_call() == [_lib.ZFFT_EINVAL] * 8 and shape[3].value == 0


def test_the_facade():
    from pypanadapter_amd import panadapter
    rows, want = _scene()
    d = tr.SCENE_DETECT
    det = panadapter.Detector(d["quantile"], d["threshold_db"], d["min_width"], d["K"], track=(1, 0, 3))
    plain = panadapter.Detector(d["quantile"], d["threshold_db"], d["min_width"], d["K"])
    for a, b in ((0, 50), (50, 51), (51, 96)):
        got = det.update(rows[a:b])
        dr.assert_same(got, tuple(w[a:b] for w in want[:3]))
        dr.assert_same(plain.update(rows[a:b]), got)  # without track= nothing changes
    with pytest.raises(ValueError):
        plain.tracks()
    rep, op, _ = tr.ref_tracks(want[1], want[2], 1, 0, 3)
    got = det.tracks()
    tr.assert_tracks_same(got, rep)
    tr.assert_tracks_same(det.open_tracks(), op)
    fs, n_fft, zoom, period = 2.4e6, 128, 4, 1e-3
    ext = det.track_extent(got, fs, n_fft, zoom, period)
    hz = det.frequencies(fs, n_fft, zoom)
    np.testing.assert_array_equal(ext["f_lo"], hz[rep["col_first"]])
    np.testing.assert_array_equal(ext["f_hi"], hz[rep["col_last"]])
    np.testing.assert_array_equal(ext["f_peak"], hz[rep["peak_col"]])
    np.testing.assert_array_equal(ext["t_start"], rep["row_first"] * period)
    np.testing.assert_array_equal(ext["t_end"], (rep["row_last"] + 1) * period)
    assert ext["t_start"][-1] == 30 * period and ext["t_end"][-1] == 80 * period
    assert ext["t_peak"][-1] == 60 * period and ext["peak_db"][-1] == np.float32(-83.0)
    det.close()
    plain.close()


# ---------------------------------------------------------------- 10. the device chain
CHAIN = dict(N=512, zoom=2, W=256, L=8192, F=2, g=1)   # 30 rows: test_gpu_detect's device case
CHAIN_DET = dict(q=0.5, thr=12.0, mw=2, K=8)
CHAIN_TRACK = (1, 1, 2)


@functools.lru_cache(maxsize=None)
def _chain_input():
    c = CHAIN
    x = war.burst_frames(c["F"], c["L"], c["N"], c["zoom"], c["W"], 9100)
    x.setflags(write=False)
    return x


def _chain_plan():
    from pypanadapter_amd import ZoomFFT
    c, d = CHAIN, CHAIN_DET
    plan = ZoomFFT(c["N"], c["zoom"], FS, n_win=c["W"], segments_per_line=c["g"])
    plan.set_detect(d["q"], d["thr"], d["mw"], d["K"])
    plan.set_track(*CHAIN_TRACK)
    return plan


def _chain_bufs(count):
    import torch
    c, K = CHAIN, CHAIN_DET["K"]
    x = torch.from_numpy(np.array(_chain_input()).view(np.float32).reshape(c["F"], c["L"], 2)).to("cuda")
    return {"x": x, "rows": stall.sentinel((count, c["W"])), "floor": stall.sentinel((count,)),
            "found": stall.sentinel((count,), torch.int32), "events": stall.sentinel((count, K, 4), torch.int32)}


def _chain_check(rows, found, events, tracks, open_tracks, state):
    from pypanadapter_amd.engine import EMISSION_DTYPE
    c, d = CHAIN, CHAIN_DET
    count = len(rows)
    want = dr.ref_detect(rows, c["W"], d["q"], d["thr"], d["mw"], d["K"])
    ev = np.ascontiguousarray(events).view(EMISSION_DTYPE).reshape(count, d["K"])
    dr.assert_same((want[0], found, ev), want[:3])
    rep, op, st = tr.ref_tracks(want[1], want[2], *CHAIN_TRACK)
    # the in-band tones of the golden recipe stay on; a burst row or two holds more than K runs, which
    # the rule defines (the first K count) and the reference follows
    assert st["open"] >= 1 and len(rep) >= 3 and st["dropped"] == 0
    tr.assert_tracks_same(tracks, rep)
    tr.assert_tracks_same(open_tracks, op)
    assert state == st


def test_device_chain_on_one_stream_without_a_host_sync():
    import torch
    c = CHAIN
    with _chain_plan() as plan:
        count = c["F"] * plan.lines(c["L"])
        assert count == 30
        b = _chain_bufs(count)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        st = side.cuda_stream
        plan.set_timing(True)
        plan.process_device(b["x"].data_ptr(), c["L"], c["F"], b["rows"].data_ptr(), st)
        plan.detect_device(b["rows"].data_ptr(), count, b["floor"].data_ptr(), b["found"].data_ptr(),
                           b["events"].data_ptr(), st)
        plan.track_push_device(b["found"].data_ptr(), b["events"].data_ptr(), count, st)
        names = plan.launch_names()
        state = plan.track_state()   # the readers wait for what is enqueued
        open_tracks, tracks = plan.open_tracks(), plan.tracks()
        assert names == ["track_label", "track_seam", "track_merge", "track_peak_row", "track_peak_col",
                         "track_count", "track_scan", "track_emit", "track_frontier"]
        assert len(plan.timings()) == len(names)
        torch.cuda.synchronize()
        _chain_check(b["rows"].cpu().numpy(), b["found"].cpu().numpy(), b["events"].cpu().numpy(), tracks,
                     open_tracks, state)


def test_device_chain_behind_a_stalled_stream():
    """process on A, detect on B, the track push on C, a second round on B, C, A -- enqueued while a
    bounded spin kernel holds A (tests/stall.py): a push that lacks its wait on the plan's earlier
    work links the sentinel, a reproducible wrong answer."""
    import torch
    streams = stall.streams()
    c = CHAIN

    def make():
        plan = _chain_plan()
        count = c["F"] * plan.lines(c["L"])
        b = _chain_bufs(count)
        warm = stall.Run(plan, streams, held=False)
        seq(plan, warm, b, rounds=1)  # the workspaces and the tracker's scratch have their size
        torch.cuda.synchronize()
        plan.detect_reset()
        plan.track_reset()
        torch.cuda.synchronize()
        return plan, _chain_bufs(count)

    def seq(plan, run, b, rounds=2):
        count = len(b["rows"])
        order = [streams[0], streams[1], streams[2], streams[1], streams[2], streams[0]]
        for k in range(rounds):
            on = order[3 * k:3 * k + 3]
            run.call(f"process{k}", plan.process_device, b["x"].data_ptr(), c["L"], c["F"], b["rows"].data_ptr(), on=on[0])
            run.call(f"detect{k}", plan.detect_device, b["rows"].data_ptr(), count, b["floor"].data_ptr(),
                     b["found"].data_ptr(), b["events"].data_ptr(), on=on[1])
            run.call(f"track_push{k}", plan.track_push_device, b["found"].data_ptr(), b["events"].data_ptr(), count,
                     on=on[2])

    def sequence(plan, run, b):
        seq(plan, run, b)
        run.check_order()
        run.expect_wait("the synchronous readers")
        state = run.host(plan.track_state)
        return {"rows": b["rows"], "found": b["found"], "events": b["events"], "state": state,
                "open": run.host(plan.open_tracks), "tracks": run.host(plan.tracks)}

    held, stepped, run = stall.enqueue_twice("track[chain]", make, sequence, streams)
    stall.same_bytes(held, stepped, "held")
    assert not (stepped["rows"] == stall.SENTINEL).any()
    # two rounds of the same 30 rows: the reference of the rows given twice
    from pypanadapter_amd.engine import EMISSION_DTYPE
    d = CHAIN_DET
    want = dr.ref_detect(stepped["rows"], c["W"], d["q"], d["thr"], d["mw"], d["K"])
    ev = np.ascontiguousarray(stepped["events"]).view(EMISSION_DTYPE).reshape(30, d["K"])
    dr.assert_same((want[0], stepped["found"], ev), want[:3])
    rep, op, st = tr.ref_tracks(np.tile(want[1], 2), np.tile(want[2], (2, 1)), *CHAIN_TRACK)
    tr.assert_tracks_same(held["tracks"], rep)
    tr.assert_tracks_same(held["open"], op)
    assert held["state"] == st and st["rows_seen"] == 60


# ---------------------------------------------------------------- 11. feature off
def test_a_plan_that_never_tracks_launches_nothing_for_it():
    from pypanadapter_amd import ZoomFFT
    rows, want = _scene()
    d = tr.SCENE_DETECT
    with ZoomFFT(128, 1, FS, n_win=128) as plan:
        plan.set_timing(True)
        plan.set_detect(d["quantile"], d["threshold_db"], d["min_width"], d["K"])
        dr.assert_same(plan.detect(rows), want[:3])
        assert plan.launch_names() == ["detect_rows"] and len(plan.timings()) == 1
        plan.set_detect_local(16, 2)
        plan.detect(rows)
        assert plan.launch_names() == ["detect_floor", "detect_rows"]
        plan.set_detect_local(0, 0)
        plan.set_track(0, 0, 1)   # on: the detect call itself is still the detector's alone
        plan.detect(rows)
        assert plan.launch_names() == ["detect_rows"]
        plan.track_push(want[1], want[2])
        assert [n for n in plan.launch_names() if not n.startswith("track_")] == []
