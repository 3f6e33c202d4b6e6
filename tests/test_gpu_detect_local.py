"""GPU checks of the row detector's local floor (zfft_plan_detect_local: per column an order
statistic of the reference cells around it) against tests/detect_local_ref.py, the rule of
include/zfft.h in numpy float32 (pinned on the CPU by test_detect_local_host.py), on the very rows
given to the device.  Everything compares with assert_array_equal -- floors and peak_db as bits,
occupancy after every call: the rule has no rounding beyond one float32 addition, so there is
no tolerance to choose.  The row lengths the issue names are set through the detector's
row-length hook, since a plan's own rows have few shapes (never one column, for one)."""
import ctypes
import functools

import numpy as np
import pytest

import detect_local_ref as dl
import detect_ref as dr
import welch_average_ref as war

pytestmark = pytest.mark.gpu
FS = war.FS
TILE = 256  # kDetectLocalTile (zfft_detect_plan.h), asserted through the hook below


def _hook(plan, name, *args):
    fn = getattr(plan.lib, name)
    fn.restype = ctypes.c_int
    return fn(plan._plan, *args)


def _local_form(plan, count):
    out = (ctypes.c_int32 * 7)()
    assert _hook(plan, "zfft__plan_detect_local_form", ctypes.c_int32(count), out) == 0
    return dict(zip(("tile", "tiles", "halo", "grid", "chunk_rows", "lds_keys", "words"), out))


def _plan(n_win, row_len=None):
    """A plan of n_win columns whose detector takes rows of row_len (default: the plan's own)."""
    from pypanadapter_amd import ZoomFFT
    n_fft = 1 << max(5, (n_win - 1).bit_length())
    plan = ZoomFFT(n_fft, 1, FS, n_win=n_win)
    if row_len is not None and row_len != plan.row_length:
        assert _hook(plan, "zfft__plan_detect_row_length", ctypes.c_int32(row_len)) == 0
    return plan


@functools.lru_cache(maxsize=None)
def _floors_ref(key, n, h, gd, q):
    """The reference floors of the cached rows `key` names, computed once per (shape, q)."""
    rows = _ROWS[key]()
    out = dl.fast_local_floors(rows, n, h, gd, q)
    out.setflags(write=False)
    return out


def _check(plan, key, n, h, gd, q, thr_db, mw, K):
    """set_detect + set_detect_local, the floors and one detect call on the rows `key` names,
    everything against the reference; returns the reference."""
    rows = _ROWS[key]()
    plan.set_detect(q, thr_db, mw, K)
    plan.set_detect_local(h, gd)
    assert plan.detect_local_shape() == (h, gd) and plan.detect_shape() == (K, plan.n_win)
    fref = _floors_ref(key, n, h, gd, q)
    fgot = plan.detect_floors(rows)
    assert fgot.dtype == np.float32 and fgot.shape == rows.shape and np.isnan(fgot[:, n:]).all()
    dl.assert_floors_same(fgot, fref, n)
    occ0, seen0 = plan.detect_occupancy()
    assert not occ0.any() and seen0 == 0  # the floors count nothing
    got = plan.detect(rows)
    want = dl.ref_detect_local(rows, n, h, gd, q, thr_db, mw, K, floors=fref)
    dr.assert_same(got, want)
    occ, seen = plan.detect_occupancy()
    assert seen == len(rows)
    np.testing.assert_array_equal(occ, want[3])
    assert not occ[n:].any()
    return want


# ---------------------------------------------------------------- 1. widths, planted runs
def _planted(count, n_win, n, seed):
    """Seeded noise around a floor that tilts 30 units over the row (sigma 1.5) with runs planted
    where the kernels have an edge: column 0, the last column, across 63|64 (an on-flag word),
    across the tile boundaries 256 k, widths 2 and 3 (min_width 3 keeps only the second), long
    runs over several words and tiles (their middle columns see only planted cells), NaN, -inf,
    +inf and -0.0 inside and beside runs, garbage beyond the row."""
    rng = np.random.default_rng(seed)
    rows = (-120.0 + 30.0 * np.arange(n_win) / n_win + 1.5 * rng.standard_normal((count, n_win))).astype(np.float32)
    level = (-70.0 + 30.0 * rng.random((count, n_win))).astype(np.float32)
    spans = [(0, 1), (n - 3, n - 1), (10, 11), (20, 22), (30, 36), (62, 65), (140, 250), (600, 900)]
    spans += [(TILE * k - 2, TILE * k + 1) for k in (1, 2, 3, 31, 255)]
    spans += [(TILE * 8 - 300, TILE * 8 + 300)]  # wider than any window: its middle is its own floor
    for a, b in spans:
        if 0 <= a <= b < n:
            rows[:, a:b + 1] = level[:, a:b + 1]
    for col, val in ((33, np.nan), (29, np.nan), (37, -np.inf), (45, np.inf), (5, -0.0), (46, 0.0), (700, np.inf),
                     (TILE * 8, np.nan)):
        if col < n:
            rows[:, col] = val
    if n > 21:
        rows[1::3, 21] = -np.inf
    rows[:, n:] = 1e30  # never read
    return rows


WIDTHS = [(1, 2), (50, 50), (64, 64), (192, 200), (257, 258), (512, 512), (2049, 2050), (8192, 8192), (65536, 65536)]
SHAPES = [(1, 0), (16, 2), (128, 128)]
QS = [0.0, 0.5, 0.75, 1.0]
_ROWS = {}


def _cached(name, make, *args):
    """_ROWS[name](): the rows make(*args) gives, built once and read-only."""
    @functools.lru_cache(maxsize=None)
    def get():
        rows = make(*args)
        rows.setflags(write=False)
        return rows
    _ROWS[name] = get


for _n, _w in WIDTHS:
    _cached(f"planted{_n}", _planted, 2 if _n >= 65536 else 4, _w, _n, 7 * _n + 1)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"h{s[0]}g{s[1]}")
@pytest.mark.parametrize("width", WIDTHS, ids=lambda w: f"n{w[0]}")
def test_exact_on_planted_rows(width, shape):
    """Every (h, guard) meets every width, the narrowest and the widest included; q walks through
    its four values so that each (h, guard) and each width sees all of them; (min_width, K) takes
    (1, 32) and (3, 1) on the same rows."""
    n, n_win = width
    h, gd = shape
    q = QS[(WIDTHS.index(width) + SHAPES.index(shape)) % 4]
    with _plan(n_win, n) as plan:
        want = None
        for mw, K in ((1, 32), (min(3, n_win), 1)):  # (min_width may not exceed n_win)
            want = _check(plan, f"planted{n}", n, h, gd, q, 12.0, mw, K)
        f = _local_form(plan, 4)
        assert f["tile"] == TILE and f["tiles"] == -(-n // TILE) and f["halo"] == h + gd
        assert f["words"] == (1 if h <= 32 else 4)
        if n >= 512 and q <= 0.5:
            assert want[3].any()  # the plants took part


@pytest.mark.parametrize("shape", [(32, 1), (33, 0), (64, 4), (65, 0), (96, 5)], ids=lambda s: f"h{s[0]}g{s[1]}")
@pytest.mark.parametrize("width", [(257, 258), (2049, 2050)], ids=lambda w: f"n{w[0]}")
def test_exact_at_the_ends_of_every_word_count(width, shape):
    """The widest half window of 1 and of 2 mask words per side, the narrowest of 2 and of 4, and
    one that leaves the fourth word half used."""
    n, n_win = width
    h, gd = shape
    with _plan(n_win, n) as plan:
        _check(plan, f"planted{n}", n, h, gd, 0.5, 12.0, 1, 32)
        assert _local_form(plan, 4)["words"] == (1 if h <= 32 else 2 if h <= 64 else 4)
        _check(plan, f"planted{n}", n, h, gd, 0.0, 12.0, 2, 8)


# ---------------------------------------------------------------- 2. windows that overhang
def _noise(count, n_win, seed):
    rng = np.random.default_rng(seed)
    rows = (-120.0 + 3.0 * rng.standard_normal((count, n_win))).astype(np.float32)
    rows[:, 3::17] += np.float32(25.0)
    return rows


_cached("noise64", _noise, 4, 64, 91)
_cached("noise512", _noise, 4, 512, 92)


@pytest.mark.parametrize("case", [(64, 30, 16, 2), (64, 36, 16, 2), (512, 300, 128, 128), (512, 512, 128, 128),
                                  (64, 2, 1, 0)], ids=str)
def test_windows_cut_at_both_ends(case):
    """row_len < 2 (h + guard) + 1: no column has its whole window."""
    n_win, n, h, gd = case
    assert n < 2 * (h + gd) + 1
    with _plan(n_win, n) as plan:
        for q in (0.5, 1.0):
            _check(plan, f"noise{n_win}", n, h, gd, q, 6.0, 1, 8)


@pytest.mark.parametrize("case", [(64, 3, 16, 2), (64, 1, 1, 0), (512, 129, 128, 128), (512, 50, 1, 128)], ids=str)
def test_rows_without_a_reference_cell(case):
    """row_len <= guard + 1: every floor is NaN, nothing is on, found is 0 and the occupancy a
    longer row left behind stays as it was."""
    n_win, n, h, gd = case
    assert n <= gd + 1
    key = f"noise{n_win}"
    rows = _ROWS[key]()
    with _plan(n_win) as plan:
        plan.set_detect(0.5, -50.0, 1, 8)  # far below everything: every column with a floor is on
        plan.set_detect_local(h, gd)
        plan.detect(rows)
        before, seen = plan.detect_occupancy()
        assert before.any() and seen == len(rows)
        assert _hook(plan, "zfft__plan_detect_row_length", ctypes.c_int32(n)) == 0
        fl = plan.detect_floors(rows)
        assert np.isnan(fl).all()
        floor, found, events = plan.detect(rows)
        dr.assert_same((floor, found, events), dl.ref_detect_local(rows, n, h, gd, 0.5, -50.0, 1, 8)[:3])
        assert not found.any() and events.tobytes() == bytes(events.nbytes)
        after, seen = plan.detect_occupancy()
        np.testing.assert_array_equal(after, before)
        assert seen == 2 * len(rows)


# ---------------------------------------------------------------- 3. dead windows inside a live row
def _dead(count, n_win, seed):
    rows = _noise(count, n_win, seed)
    rows[:, 100:160] = np.nan      # longer than 2 (16 + 2) + 1 = 37
    rows[:, 300:360] = -np.inf
    rows[:, 400] = np.inf          # left out of its neighbours' populations, itself on
    rows[:, 405:407] = np.inf
    rows[:, 256] = np.inf          # at a tile boundary
    return rows


_cached("dead512", _dead, 4, 512, 93)


@pytest.mark.parametrize("shape", [(1, 0), (16, 2)], ids=str)
@pytest.mark.parametrize("q", [0.0, 0.5, 1.0])
def test_dead_windows_inside_a_live_row(shape, q):
    h, gd = shape
    with _plan(512) as plan:
        floor, found, events, occ = _check(plan, "dead512", 512, h, gd, q, 6.0, 1, 32)
        fl = _floors_ref("dead512", 512, h, gd, q)
        for a, b in ((100, 160), (300, 360)):  # the middle of each stretch has no finite cell
            mid = slice(a + h + gd, b - h - gd)
            assert np.isnan(fl[:, mid]).all() and not occ[mid].any()
            assert np.isfinite(fl[:, a - 1]).all() and np.isfinite(fl[:, b]).all()  # the flanks have floors
        assert np.isfinite(fl[:, 399:408]).all()
        assert occ[400] == occ[405] == occ[406] == occ[256] == 4  # +inf is on wherever its floor is finite
        assert np.isfinite(floor).all()  # the row-global floor is untouched by the stretches


# ---------------------------------------------------------------- 4. ties
def _ties(count, n_win, seed):
    rng = np.random.default_rng(seed)
    rows = (np.round(2.0 * (-120.0 + 4.0 * rng.standard_normal((count, n_win)))) / 2.0).astype(np.float32)
    rows[-3] = np.float32(-97.25)
    rows[-2] = 0.0
    rows[-1] = -0.0
    return rows


_cached("ties512", _ties, 6, 512, 94)
_cached("ties200", _ties, 6, 200, 95)


@pytest.mark.parametrize("width", [(512, 512), (192, 200)], ids=str)
@pytest.mark.parametrize("q", QS)
def test_ties_and_constant_rows(width, q):
    n, n_win = width
    with _plan(n_win, n) as plan:
        for (h, gd), thr_db in (((16, 2), 1.5), ((128, 128), 0.0), ((1, 0), -1.0)):
            floor, found, events, occ = _check(plan, f"ties{n_win}", n, h, gd, q, thr_db, 1, 8)
            fl = _floors_ref(f"ties{n_win}", n, h, gd, q)
            lone = np.isnan(fl[-3, :n])  # (columns without a reference cell: none unless the row is short)
            assert np.all(fl[-3, :n][~lone] == np.float32(-97.25)) and np.all(fl[-2:, :n][:, ~lone] == 0.0)
            if thr_db <= 0.0:
                assert found[-1] >= 1 and occ[:n][~lone].min() >= 3  # a constant row is on against itself


# ---------------------------------------------------------------- 5. mode switching on one plan
def test_mode_switching_on_one_plan():
    from pypanadapter_amd import _lib
    from pypanadapter_amd.engine import EMISSION_DTYPE
    rows = _ROWS["planted512"]()
    n = 512
    q, thr_db, mw, K = 0.5, 12.0, 1, 32
    gwant = dr.ref_detect(rows, n, q, thr_db, mw, K)
    with _plan(512) as plan:
        lib, P = plan.lib, plan._plan
        hw, gd = ctypes.c_int32(-1), ctypes.c_int32(-1)
        out = np.zeros_like(rows)
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

        def floor_calls():  # (refused before anything is read: only ever called where they must be)
            return [lib.zfft_detect_floors(P, ptr(rows), len(rows), ptr(out)),
                    lib.zfft_detect_floors_device(P, ctypes.c_void_p(16), 1, ctypes.c_void_p(16), None)]

        def new_calls():  # with detection off
            return [lib.zfft_plan_detect_local(P, 16, 2),
                    lib.zfft_detect_local_shape(P, ctypes.byref(hw), ctypes.byref(gd))] + floor_calls()

        assert new_calls() == [_lib.ZFFT_EINVAL] * 4 and (hw.value, gd.value) == (0, 0)  # detection is off
        plan.set_timing(True)
        plan.set_detect(q, thr_db, mw, K)
        assert plan.detect_local_shape() == (0, 0)
        assert floor_calls() == [_lib.ZFFT_EINVAL] * 2  # global: no floors
        plan.set_detect_local(0, 0)
        assert floor_calls() == [_lib.ZFFT_EINVAL] * 2
        for bad in ((0, 1), (-1, 0), (129, 0), (16, -1), (16, 129)):
            with pytest.raises(ValueError):
                plan.set_detect_local(*bad)
        assert plan.detect_local_shape() == (0, 0)
        first = plan.detect(rows)
        assert plan.launch_names() == ["detect_rows"]
        dr.assert_same(first, gwant)
        np.testing.assert_array_equal(plan.detect_occupancy()[0], gwant[3])

        plan.set_detect_local(16, 2)
        occ, seen = plan.detect_occupancy()
        assert not occ.any() and seen == 0  # zeroed by the switch
        local = plan.detect(rows)
        assert plan.launch_names() == ["detect_floor", "detect_rows"] and len(plan.timings()) == 2
        lwant = dl.ref_detect_local(rows, n, 16, 2, q, thr_db, mw, K)
        dr.assert_same(local, lwant)
        np.testing.assert_array_equal(plan.detect_occupancy()[0], lwant[3])
        assert not np.array_equal(lwant[3], gwant[3])  # the two rules differ on these rows
        plan.detect_floors(rows)
        assert plan.launch_names() == ["detect_floor"]
        plan.set_detect(q, thr_db, mw, K)  # a setter call on a plan that is on keeps the mode
        assert plan.detect_local_shape() == (16, 2)
        dr.assert_same(plan.detect(rows), lwant)

        plan.set_detect_local(0)
        occ, seen = plan.detect_occupancy()
        assert not occ.any() and seen == 0
        second = plan.detect(rows)
        assert plan.launch_names() == ["detect_rows"]
        dr.assert_same(second, first)
        for a, b in zip(first, second):
            assert a.tobytes() == b.tobytes()
        np.testing.assert_array_equal(plan.detect_occupancy()[0], gwant[3])

        plan.set_detect_local(128, 128)
        plan.set_detect(max_per_row=0)  # off ...
        assert new_calls() == [_lib.ZFFT_EINVAL] * 4
        plan.set_detect(q, thr_db, mw, K)  # ... and on: global again
        assert plan.detect_local_shape() == (0, 0)
        dr.assert_same(plan.detect(rows), gwant)
        ev = np.zeros((len(rows), K), EMISSION_DTYPE)
        assert ev.itemsize == 16  # the record layout stays


# ---------------------------------------------------------------- 6. splits and streams
_cached("many512", _noise, 300, 512, 96)


def test_many_rows_in_one_call_and_in_three():
    rows = _ROWS["many512"]()
    h, gd, q = 16, 2, 0.5
    with _plan(512) as plan:
        want = _check(plan, "many512", 512, h, gd, q, 6.0, 1, 8)
        fref = _floors_ref("many512", 512, h, gd, q)
        plan.detect_reset()
        cuts = [0, 100, 101, len(rows)]
        parts = [plan.detect(rows[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
        dr.assert_same(tuple(np.concatenate([p[i] for p in parts]) for i in range(3)), want)
        occ, seen = plan.detect_occupancy()
        assert seen == len(rows)
        np.testing.assert_array_equal(occ, want[3])
        fparts = np.concatenate([plan.detect_floors(rows[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
        dl.assert_floors_same(fparts, fref, 512)


def test_device_rows_on_the_same_stream_and_beside_persistence():
    """process_device into a torch buffer, then detect_device in local mode and
    detect_floors_device on that buffer on the same stream: the results are the reference's on
    the rows copied back.  Persistence and detection on one plan give what each gives alone."""
    import torch
    import persistence_ref as pr
    from pypanadapter_amd import ZoomFFT
    from pypanadapter_amd.engine import EMISSION_DTYPE
    N, zoom, W, L, F, g = 512, 2, 256, 8192, 2, 1
    x = war.burst_frames(F, L, N, zoom, W, 9100)
    dev = torch.device("cuda:0")
    xd = torch.from_numpy(np.array(x).view(np.float32).reshape(F, L, 2)).to(dev)
    K, q, thr_db, mw, h, gd = 8, 0.5, 12.0, 2, 16, 2
    levels, lo, hi = 96, -200.0, -8.0

    def run(persist):
        with ZoomFFT(N, zoom, FS, n_win=W, segments_per_line=g) as plan:
            count = F * plan.lines(L)
            plan.set_timing(True)
            plan.set_detect(q, thr_db, mw, K)
            plan.set_detect_local(h, gd)
            if persist:
                plan.set_persistence(levels, lo, hi)
            rows = torch.empty((count, W), device=dev, dtype=torch.float32)
            floors = torch.full((count, W), 7.0, device=dev, dtype=torch.float32)
            floor = torch.empty(count, device=dev, dtype=torch.float32)
            found = torch.empty(count, device=dev, dtype=torch.int32)
            events = torch.empty((count, K, 4), device=dev, dtype=torch.int32)
            st = torch.cuda.current_stream().cuda_stream
            plan.process_device(xd.data_ptr(), L, F, rows.data_ptr(), st)
            if persist:
                plan.persistence_push_device(rows.data_ptr(), count, st)
            plan.detect_device(rows.data_ptr(), count, floor.data_ptr(), found.data_ptr(), events.data_ptr(), st)
            names = plan.launch_names()
            plan.detect_floors_device(rows.data_ptr(), count, floors.data_ptr(), st)
            names2 = plan.launch_names()
            out = {"hist": plan.persistence()[0] if persist else None, "occ": plan.detect_occupancy(),
                   "names": names, "names2": names2}
            torch.cuda.synchronize()
            out["rows"], out["floors"] = rows.cpu().numpy(), floors.cpu().numpy()
            out["got"] = (floor.cpu().numpy(), found.cpu().numpy(),
                          events.cpu().numpy().view(EMISSION_DTYPE).reshape(count, K))
            return out

    both, det = run(True), run(False)
    assert len(both["rows"]) == 30 and both["rows"].tobytes() == det["rows"].tobytes()
    fref = dl.ref_local_floors(both["rows"], W, h, gd, q)
    want = dl.ref_detect_local(both["rows"], W, h, gd, q, thr_db, mw, K, floors=fref)
    assert want[1].sum() > 0 and want[3].any()
    for out in (both, det):
        dr.assert_same(out["got"], want)
        dl.assert_floors_same(out["floors"], fref, W)
        np.testing.assert_array_equal(out["occ"][0], want[3])
        assert out["occ"][1] == 30
        assert out["names"] == ["detect_floor", "detect_rows"] and out["names2"] == ["detect_floor"]
    np.testing.assert_array_equal(both["hist"], pr.ref_hist(both["rows"], levels, lo, hi, W))


# ---------------------------------------------------------------- 7. passes through a small scratch
def test_passes_through_a_small_scratch():
    rows = _ROWS["many512"]()[:50]
    h, gd, q = 16, 2, 0.75
    with _plan(512) as plan:
        plan.set_timing(True)
        plan.set_detect(q, 6.0, 2, 8)
        plan.set_detect_local(h, gd)
        whole = plan.detect(rows)
        assert plan.launch_names() == ["detect_floor", "detect_rows"]
        occ_whole = plan.detect_occupancy()[0]
        fwhole = plan.detect_floors(rows)
        plan.detect_reset()
        assert _hook(plan, "zfft__plan_detect_local_cap", ctypes.c_int64(512 * 4 * 7)) == 0
        assert _local_form(plan, 50)["chunk_rows"] == 7
        parts = plan.detect(rows)
        assert plan.launch_names() == ["detect_floor", "detect_rows"] * 8  # 7 passes of 7 rows and one of 1
        dr.assert_same(parts, whole)
        np.testing.assert_array_equal(plan.detect_occupancy()[0], occ_whole)
        fparts = plan.detect_floors(rows)
        assert plan.launch_names() == ["detect_floor"]
        assert fparts.tobytes() == fwhole.tobytes()
        fref = dl.ref_local_floors(rows, 512, h, gd, q)
        dl.assert_floors_same(fwhole, fref, 512)
        dr.assert_same(whole, dl.ref_detect_local(rows, 512, h, gd, q, 6.0, 2, 8, floors=fref))


# ---------------------------------------------------------------- 8. meaning
@pytest.mark.parametrize("case", dl.MEANING_LOCAL["rows"], ids=lambda c: f"n{c[0]}")
def test_planted_tones_on_a_tilted_floor(case):
    """A floor rising 40 units over the row with tones 20 units above it: the local detector
    reports exactly the tones, the global one (q = 0.5) 21 / 6 runs without the two tones of the
    quiet part and with a last run up to column n - 1 (the input's condition is checked without a
    GPU by test_detect_local_host.py)."""
    n, tones = case
    c = dl.MEANING_LOCAL
    v = dl.meaning_row(n, tones)[None, :]
    with _plan(n) as plan:
        assert plan.row_length == n
        plan.set_detect(0.5, c["threshold_db"], c["min_width"], c["K"])
        _, found, ev = plan.detect(v)
        assert found[0] == c["global_runs"][n]
        runs = [(int(e["first"]), int(e["last"])) for e in ev[0, :found[0]]]
        for t in c["global_misses"][n]:
            assert not any(a <= t + 1 and b >= t for a, b in runs)
        assert runs[-1][1] == n - 1
        for h, gd, q in c["shapes"]:
            plan.set_detect(q, c["threshold_db"], c["min_width"], c["K"])
            plan.set_detect_local(h, gd)
            got = plan.detect(v)
            dr.assert_same(got, dl.ref_detect_local(v, n, h, gd, q, c["threshold_db"], c["min_width"], c["K"]))
            _, found, ev = got
            assert [(int(e["first"]), int(e["last"])) for e in ev[0, :found[0]]] == [(t, t + 1) for t in tones]
            assert all(t <= int(e["peak"]) <= t + 1 for e, t in zip(ev[0], tones))
            occ, _ = plan.detect_occupancy()
            assert occ.sum() == 2 * len(tones)


# ---------------------------------------------------------------- 9. the facade
def test_the_facade_over_psd_lines():
    from pypanadapter_amd import panadapter
    N, zoom = 256, 1
    rng = np.random.default_rng(77)
    L = N * 6
    x = ((rng.standard_normal(L) + 1j * rng.standard_normal(L)) / np.sqrt(2.0)
         + 0.5 * np.exp(2j * np.pi * 40 * np.arange(L) / N)).astype(np.complex64)
    rows = panadapter.psd_lines(x, FS, N, zoom, 1)
    assert rows.ndim == 2 and rows.shape[1] == N and len(rows) >= 4
    det = panadapter.Detector(quantile=0.5, threshold_db=12.0, min_width=1, max_per_row=8, local=(16, 2))
    with pytest.raises(AttributeError):
        det.occupancy()
    got = det.update(rows)
    r32 = rows.astype(np.float32)
    fref = dl.ref_local_floors(r32, N, 16, 2, 0.5)
    want = dl.ref_detect_local(r32, N, 16, 2, 0.5, 12.0, 1, 8, floors=fref)
    dr.assert_same(got, want)
    assert det.occupancy()[N // 2 + 40] == 1.0  # the tone's column, in every line
    np.testing.assert_array_equal(det.occupancy(), want[3][:N] / float(len(rows)))
    fl = det.floors(rows)
    assert fl.shape == (len(rows), N) and fl.dtype == np.float32
    dl.assert_floors_same(fl, fref, N)
    assert det.rows_seen == len(rows)  # the floors count nothing
    odd = r32[:, :51]  # an odd width gets a NaN column and loses nothing
    dr.assert_same(det.update(odd), dl.ref_detect_local(odd, 51, 16, 2, 0.5, 12.0, 1, 8))
    assert det.floors(odd).shape == (len(rows), 51)
    det.close()
    plain = panadapter.Detector(threshold_db=12.0)
    plain.update(rows)
    with pytest.raises(ValueError):
        plain.floors(rows)  # the row-global floor has none
    plain.close()
