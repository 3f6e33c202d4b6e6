"""GPU checks of the row detector (zfft_plan_detect: per row a noise floor, the emissions above
floor + threshold, per column an occupancy count) against detect_ref.ref_detect, the rule of
include/zfft.h in numpy float32 (pinned on the CPU by test_detect_host.py), on the very rows
given to the device.  Floors, counts, records (peak_db as bits) and occupancy compare exactly:
the rule has no rounding beyond one float32 addition, so there is no tolerance to choose.  Only
the comparison against the float64 Welch reference (test 6) has a bound, the row gate DB_TOL on
the floor; its columns are exact because the input keeps every value 0.01 units away from the
threshold (checked without a GPU by test_detect_host.py)."""
import ctypes
import functools

import numpy as np
import pytest

import detect_ref as dr
import welch_average_ref as war
from conftest import DB_TOL

pytestmark = pytest.mark.gpu
FS = war.FS


def _form(plan, count):
    """(waves, per, grid) of a call on `count` rows of this plan (hook zfft__plan_detect_form)."""
    hook = plan.lib.zfft__plan_detect_form
    hook.argtypes = [ctypes.c_void_p, ctypes.c_int32] + [ctypes.POINTER(ctypes.c_int32)] * 3
    hook.restype = ctypes.c_int
    w, p, g = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    assert hook(plan._plan, count, ctypes.byref(w), ctypes.byref(p), ctypes.byref(g)) == 0
    return w.value, p.value, g.value


def _check(plan, rows, n, q, thr_db, mw, K):
    """set_detect, one detect call on `rows`, everything against the reference; returns it."""
    plan.set_detect(q, thr_db, mw, K)
    assert plan.detect_shape() == (K, plan.n_win)
    got = plan.detect(rows)
    want = dr.ref_detect(rows, n, q, thr_db, mw, K)
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32 and got[2].shape == (len(rows), K)
    dr.assert_same(got, want)
    occ, seen = plan.detect_occupancy()
    assert occ.dtype == np.uint32 and occ.shape == (plan.n_win,) and seen == len(rows)
    np.testing.assert_array_equal(occ, want[3])
    assert not occ[n:].any()
    return want


# ---------------------------------------------------------------- 1. widths, planted runs
WIDTHS = {"w64_one_word": (64, 64, "complex64"), "w50_masked_word": (64, 50, "complex64"),
          "w200_masked_tail": (256, 200, "complex64"), "w512_cfg2": (512, 512, "complex64"),
          "w301_real_short_rows": (1024, 301, "f32"), "w8192": (8192, 8192, "complex64"),
          "w65536": (65536, 65536, "complex64")}


def _planted(count, n_win, n, waves, per, seed):
    """Seeded noise around -120 (sigma 1.5: the floor + 12 stands 8 sigma out) with runs planted
    where the kernel has an edge: column 0, the last valid column, across 63|64, across the
    per-lane chunk boundaries 64 * waves * i and a wave boundary inside a chunk, widths 2 and 3
    (min_width 3 keeps only the second), NaN and -inf inside and beside runs, long runs over
    several words, and garbage beyond row_length.  Returns (rows, columns the plants cover)."""
    rng = np.random.default_rng(seed)
    rows = (-120.0 + 1.5 * rng.standard_normal((count, n_win))).astype(np.float32)
    level = (-70.0 + 30.0 * rng.random((count, n_win))).astype(np.float32)  # distinct peaks
    spans = [(0, 1), (n - 3, n - 1), (10, 11), (20, 22), (30, 36)]
    if n > 70:
        spans.append((62, 65))
    chunk = 64 * waves
    bounds = sorted({chunk * i for i in (1, 2, per // 2, per - 1) if 0 < chunk * i < n - 2})
    if waves > 1 and 64 * (waves + 1) < n - 2:
        bounds.append(64 * (waves + 1))  # a wave boundary that is no chunk boundary
    for b in bounds:
        spans.append((b - 2, b + 1))
    if n > 400:
        spans.append((140, 250))  # over two word boundaries
    if n > 1000:
        spans.append((600, 900))  # over five words, three of them full
    covered = np.zeros(n_win, dtype=bool)
    for a, b in spans:
        assert 0 <= a <= b < n
        rows[:, a:b + 1] = level[:, a:b + 1]
        covered[a:b + 1] = True
    rows[:, 33] = np.nan        # inside (30, 36): two runs of three
    rows[:, 29] = np.nan        # beside it
    rows[:, 37] = -np.inf
    rows[1::3, 21] = -np.inf    # inside (20, 22) on every third row: two runs of one
    rows[:, n:] = 1e30          # never read
    if count > 4:
        rows[3, :n] = np.nan                    # no finite value at all
        rows[4, :n] = np.float32(-120.0)        # one constant: floor + 12 is above everything
    return rows, covered


@functools.lru_cache(maxsize=None)
def _planted_for(width, waves, per):
    N, W, dtype = WIDTHS[width]
    n = 151 if dtype == "f32" else W
    rows, covered = _planted(3 if W >= 65536 else 37, W, n, waves, per, 7 * W + 1)
    rows.setflags(write=False)
    return rows, covered


@pytest.mark.parametrize("K", [1, 8, 32])
@pytest.mark.parametrize("min_width", [1, 3])
@pytest.mark.parametrize("width", list(WIDTHS))
def test_exact_on_planted_rows(width, min_width, K):
    from pypanadapter_amd import ZoomFFT
    N, W, dtype = WIDTHS[width]
    with ZoomFFT(N, 1, FS, n_win=W, in_dtype=dtype) as plan:
        n = plan.row_length
        assert n == (151 if dtype == "f32" else W)
        count = 3 if W >= 65536 else 37
        waves, per, grid = _form(plan, count)
        assert 64 * waves * per >= n and grid == count
        rows, covered = _planted_for(width, waves, per)
        floor, found, events, occ = _check(plan, rows, n, 0.5, 12.0, min_width, K)
        # the plants are what was found: nothing else is on, and the edge cases took part
        planted = len(rows) - (2 if len(rows) > 4 else 0)  # (rows 3 and 4 are the NaN and the constant row)
        assert np.all(np.abs(floor[:3] + 120.0) < 3.0)
        assert found[0] >= (6 if min_width == 1 else 4) and found.max() > 1
        assert not occ[:n][~covered[:n]].any() and occ[n - 1] == planted and occ[33] == 0
        assert events[0, 0]["first"] == (0 if min_width == 1 else 20)
        assert occ[0] == occ[10] == (planted if min_width == 1 else 0)  # the runs of width 2
        # cropped rows (as rows() returns them) are padded on the host: the same again
        plan.detect_reset()
        got = plan.detect(rows[:, :n])
        dr.assert_same(got, (floor, found, events))
        np.testing.assert_array_equal(plan.detect_occupancy()[0], occ)


# the other end of every form's domain (zfft_detect_plan.h): with WIDTHS, each form the chooser
# can pick runs at its smallest and at its largest even width
FORM_ENDS = {"w128": (128, 128), "w130": (256, 130), "w256": (256, 256), "w258": (512, 258), "w514": (1024, 514),
             "w2048": (2048, 2048), "w2050": (4096, 2050), "w8194": (16384, 8194)}


@pytest.mark.parametrize("width", list(FORM_ENDS))
def test_exact_at_the_ends_of_every_form(width):
    from pypanadapter_amd import ZoomFFT
    N, W = FORM_ENDS[width]
    with ZoomFFT(N, 1, FS, n_win=W) as plan:
        waves, per, _ = _form(plan, 11)
        with ZoomFFT(N, 1, FS, n_win=W - 2) as narrower:
            below = _form(narrower, 11)[:2]
        assert 64 * waves * per == W or below != (waves, per)  # the form's largest or smallest even width
        rows, covered = _planted(11, W, W, waves, per, 13 * W + 5)
        for mw, K in ((3, 8), (1, 32)):
            _, found, _, occ = _check(plan, rows, W, 0.5, 12.0, mw, K)
            assert found[0] >= 4 and not occ[~covered].any()
            plan.detect_reset()


# ---------------------------------------------------------------- 2. ties and signs
@pytest.mark.parametrize("width", ["w200_masked_tail", "w512_cfg2", "w8192"])
@pytest.mark.parametrize("q", [0.0, 0.25, 0.5, 1.0])
def test_ties_constants_and_signs(width, q):
    from pypanadapter_amd import ZoomFFT
    N, W, _ = WIDTHS[width]
    rng = np.random.default_rng(300 + W)
    count = 12
    quant = (np.round(2.0 * (-120.0 + 4.0 * rng.standard_normal((count, W)))) / 2.0).astype(np.float32)
    assert np.mean(quant == np.median(quant, axis=1, keepdims=True)) > 0.03  # hundreds of ties at the floor
    const = np.full((3, W), -97.25, dtype=np.float32)
    const[1] = 0.0
    const[2] = -0.0
    mixed = (50.0 * rng.standard_normal((count, W))).astype(np.float32)
    mixed[:, ::7] = 0.0
    mixed[:, 3::7] = -0.0
    mixed[:, 5::11] = np.float32(1e-42)   # denormals of both signs
    mixed[:, 6::13] = np.float32(-1e-42)
    with ZoomFFT(N, 1, FS, n_win=W) as plan:
        _check(plan, quant, W, q, 1.5, 1, 8)
        _check(plan, quant, W, q, -1.0, 3, 32)  # a negative threshold
        floor, found, events, occ = _check(plan, const, W, q, 0.0, 1, 8)
        np.testing.assert_array_equal(found, [1, 1, 1])  # everything is on: one run of n columns
        assert all(events[i, 0]["first"] == 0 and events[i, 0]["last"] == W - 1 and events[i, 0]["peak"] == 0
                   for i in range(3))
        np.testing.assert_array_equal(occ, np.full(W, 3, dtype=np.uint32))
        _check(plan, mixed, W, q, 0.0, 1, 32)
        _check(plan, mixed, W, q, -20.0, 2, 8)
        _check(plan, mixed, W, q, 30.0, 1, 1)


# ---------------------------------------------------------------- 3. the cap
@pytest.mark.parametrize("width", ["w50_masked_word", "w512_cfg2", "w8192"])
@pytest.mark.parametrize("K", [1, 8, 32])
def test_cap_on_alternating_rows(width, K):
    from pypanadapter_amd import ZoomFFT
    N, W, _ = WIDTHS[width]
    rows = np.full((5, W), -120.0, dtype=np.float32)
    rows[:, 1::2] = np.linspace(-60.0, -40.0, W // 2, dtype=np.float32)[None, :]
    rows[:, 0::2] -= np.float32(0.5) * np.arange(W // 2, dtype=np.float32)[None, :] / (W // 2)  # the floor is off
    with ZoomFFT(N, 1, FS, n_win=W) as plan:
        floor, found, events, occ = _check(plan, rows, W, 0.25, 12.0, 1, K)
        np.testing.assert_array_equal(found, np.full(5, W // 2))
        nrec = min(K, W // 2)
        np.testing.assert_array_equal(events["first"][:, :nrec], np.tile(1 + 2 * np.arange(nrec), (5, 1)))
        assert events[:, nrec:].tobytes() == bytes(events[:, nrec:].nbytes)
        np.testing.assert_array_equal(occ[1::2], np.full(W // 2, 5))  # the runs beyond the cap too
        assert not occ[0::2].any()


# ---------------------------------------------------------------- 4. many rows
@functools.lru_cache(maxsize=None)
def _concentrated():
    """20,000 x 128 rows: 90 % of each row's values within 3 units of its floor near -120 (the
    flat floor of a quiet band), the rest anywhere in [-135, -3], so about a dozen columns of a
    row are on."""
    count, W = 20000, 128
    rng = np.random.default_rng(4242)
    near = -121.5 + 3.0 * rng.random((count, W))
    wide = rng.uniform(-135.0, -3.0, (count, W))
    rows = np.where(rng.random((count, W)) < 0.9, near, wide).astype(np.float32)
    ref = dr.ref_detect(rows, W, 0.5, 12.0, 1, 8)
    assert np.all(np.abs(ref[0] + 120.0) < 1.6) and 5 < ref[1].mean() < 15
    rows.setflags(write=False)
    for a in ref:
        a.setflags(write=False)
    return rows, ref


def test_many_rows_in_one_call_and_in_three():
    from pypanadapter_amd import ZoomFFT
    rows, ref = _concentrated()
    with ZoomFFT(128, 1, FS, n_win=128) as plan:
        plan.set_timing(True)
        plan.set_detect(0.5, 12.0, 1, 8)
        got = plan.detect(rows)
        assert plan.launch_names() == ["detect_rows"] and len(plan.timings()) == 1
        assert _form(plan, len(rows))[2] < len(rows)  # more than one row per workgroup
        dr.assert_same(got, ref)
        occ, seen = plan.detect_occupancy()
        assert seen == len(rows)
        np.testing.assert_array_equal(occ, ref[3])
        plan.detect_reset()
        occ, seen = plan.detect_occupancy()
        assert not occ.any() and seen == 0
        cuts = [0, 7000, 7001, len(rows)]
        parts = [plan.detect(rows[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
        dr.assert_same(tuple(np.concatenate([p[i] for p in parts]) for i in range(3)), ref)
        occ, seen = plan.detect_occupancy()
        assert seen == len(rows)
        np.testing.assert_array_equal(occ, ref[3])


# ---------------------------------------------------------------- 5. device path and streams
def test_device_rows_on_the_same_stream_and_beside_persistence():
    """process_device with one line per segment into a torch buffer, then detect_device on that
    buffer on the same stream: the results are ref_detect of the rows copied back.  Persistence
    and detection on one plan give the tables each gives alone."""
    import torch
    import persistence_ref as pr
    from pypanadapter_amd import ZoomFFT
    from pypanadapter_amd.engine import EMISSION_DTYPE
    N, zoom, W, L, F, g = 512, 2, 256, 8192, 2, 1  # stockham_n512_zoom2
    x = war.burst_frames(F, L, N, zoom, W, 9100)
    dev = torch.device("cuda:0")
    xd = torch.from_numpy(np.array(x).view(np.float32).reshape(F, L, 2)).to(dev)
    K, q, thr_db, mw = 8, 0.5, 12.0, 2
    levels, lo, hi = 96, -200.0, -8.0

    def run(detect, persist):
        with ZoomFFT(N, zoom, FS, n_win=W, segments_per_line=g) as plan:
            R = plan.lines(L)
            count = F * R
            plan.set_timing(True)
            if detect:
                plan.set_detect(q, thr_db, mw, K)
            if persist:
                plan.set_persistence(levels, lo, hi)
            rows = torch.empty((count, W), device=dev, dtype=torch.float32)
            floor = torch.empty(count, device=dev, dtype=torch.float32)
            found = torch.empty(count, device=dev, dtype=torch.int32)
            events = torch.empty((count, K, 4), device=dev, dtype=torch.int32)
            st = torch.cuda.current_stream().cuda_stream
            plan.process_device(xd.data_ptr(), L, F, rows.data_ptr(), st)
            names = []
            if persist:
                plan.persistence_push_device(rows.data_ptr(), count, st)
            if detect:
                plan.detect_device(rows.data_ptr(), count, floor.data_ptr(), found.data_ptr(), events.data_ptr(), st)
                names = plan.launch_names()
            out = {"hist": plan.persistence()[0] if persist else None,
                   "occ": plan.detect_occupancy() if detect else None, "names": names}
            torch.cuda.synchronize()
            out["rows"] = rows.cpu().numpy()
            if detect:
                out["got"] = (floor.cpu().numpy(), found.cpu().numpy(),
                              events.cpu().numpy().view(EMISSION_DTYPE).reshape(count, K))
            return out

    both, det, per = run(True, True), run(True, False), run(False, True)
    assert len(both["rows"]) == 30 and both["rows"].tobytes() == det["rows"].tobytes() == per["rows"].tobytes()
    want = dr.ref_detect(both["rows"], W, q, thr_db, mw, K)
    assert want[1].sum() >= 30 and want[3].any()  # the in-band tones of the golden recipe
    for out in (both, det):
        dr.assert_same(out["got"], want)
        np.testing.assert_array_equal(out["occ"][0], want[3])
        assert out["occ"][1] == 30 and "detect_rows" in out["names"]
    np.testing.assert_array_equal(both["hist"], per["hist"])
    np.testing.assert_array_equal(per["hist"], pr.ref_hist(per["rows"], levels, lo, hi, W))


# ---------------------------------------------------------------- 6. meaning
def test_planted_tones_are_the_emissions(oracle_lib):
    """Three complex tones of unequal strength over seeded noise (detect_ref.MEANING), one mean
    row of 17 segments per frame, threshold 12 units = 4x in power.  The reference rule on the
    float64 rows finds exactly the three tones and no reference value lies within 0.01 units of
    the threshold (ten times the row gate; the same conditions are checked without a GPU in
    test_detect_host.py), so the device's columns must be the reference's, its peaks map to the
    tones' frequencies within half a bin and its floor is within DB_TOL of the reference's."""
    from pypanadapter_amd import panadapter
    c = dr.MEANING
    x = dr.meaning_frames()
    ref_rows = np.stack([war.ref_row(x[f], c["fs"], c["N"], c["zoom"], c["W"], "mean") for f in range(c["F"])])
    rfloor, rfound, rev, _ = dr.ref_detect(ref_rows.astype(np.float32), c["W"], 0.5, c["threshold_db"], 1, 8)
    floor64 = np.sort(ref_rows, axis=1)[:, (c["W"] - 1) // 2]
    assert np.abs(ref_rows - (floor64 + c["threshold_db"])[:, None]).min() > 0.01
    np.testing.assert_array_equal(rfound, [3] * c["F"])
    rows = np.stack([panadapter.psd_row(x[f], c["fs"], c["N"], c["zoom"]) for f in range(c["F"])])
    assert rows.shape == ref_rows.shape
    det = panadapter.Detector(quantile=0.5, threshold_db=c["threshold_db"], min_width=1, max_per_row=8, fs=c["fs"])
    floor, found, ev = det.update(rows)
    np.testing.assert_array_equal(found, rfound)
    for name in ("first", "last", "peak"):
        np.testing.assert_array_equal(ev[name], rev[name], err_msg=name)
    hz = det.frequencies(c["fs"], c["N"], c["zoom"])
    bin_hz = c["fs"] / (c["zoom"] * c["N"])
    for f in range(c["F"]):
        for r, (b, _) in enumerate(c["tones"]):
            assert abs(hz[ev[f, r]["peak"]] - b * bin_hz) <= 0.5 * bin_hz
    print("floor error", np.abs(floor.astype(np.float64) - floor64).max())
    assert np.abs(floor.astype(np.float64) - floor64).max() <= DB_TOL
    np.testing.assert_allclose(det.occupancy(), dr.ref_detect(rows, c["W"], 0.5, c["threshold_db"], 1, 8)[3] / 3.0)
    det.close()


# ---------------------------------------------------------------- 7. off and errors
def test_off_errors_and_the_facade():
    from pypanadapter_amd import ZoomFFT, _lib, panadapter
    from pypanadapter_amd.engine import EMISSION_DTYPE
    W = 64
    rows = (-120.0 + np.random.default_rng(5).standard_normal((9, W))).astype(np.float32)
    rows[:, 20:23] = -50.0
    with ZoomFFT(64, 1, FS, n_win=W) as plan:
        plan.set_timing(True)
        lib, P = plan.lib, plan._plan
        fl, fo, ev = np.zeros(9, np.float32), np.zeros(9, np.int32), np.zeros((9, 8), EMISSION_DTYPE)
        occ, seen, k, cols = np.zeros(W, np.uint32), ctypes.c_uint64(), ctypes.c_int32(-1), ctypes.c_int32(-1)
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

        def every_call():
            return [lib.zfft_detect(P, ptr(rows), 9, ptr(fl), ptr(fo), ptr(ev)),
                    lib.zfft_detect_device(P, ctypes.c_void_p(16), 1, ctypes.c_void_p(16), ctypes.c_void_p(16),
                                           ctypes.c_void_p(16), None),
                    lib.zfft_detect_occupancy(P, ptr(occ), ctypes.byref(seen)),
                    lib.zfft_detect_reset(P),
                    lib.zfft_detect_shape(P, ctypes.byref(k), ctypes.byref(cols))]

        assert every_call() == [_lib.ZFFT_EINVAL] * 5 and k.value == 0  # off by default
        for bad in ((0.5, 12.0, 1, 33), (0.5, 12.0, 1, -1), (-0.01, 12.0, 1, 8), (1.01, 12.0, 1, 8),
                    (float("nan"), 12.0, 1, 8), (0.5, float("inf"), 1, 8), (0.5, float("nan"), 1, 8),
                    (0.5, 12.0, 0, 8), (0.5, 12.0, W + 1, 8)):
            with pytest.raises(ValueError):
                plan.set_detect(*bad)
        assert every_call() == [_lib.ZFFT_EINVAL] * 5  # a refused setting enables nothing
        plan.rows(np.zeros(64 + 32 * 10, dtype=np.complex64))
        assert "detect_rows" not in plan.launch_names()  # a plan that never enabled it launches nothing for it
        plan.set_detect(0.5, 12.0, W, 8)  # min_width = n_win is allowed
        assert plan.detect(rows)[1].tolist() == [0] * 9
        plan.set_detect(0.5, 12.0, 1, 8)  # re-enabled: zeros
        occ0, seen0 = plan.detect_occupancy()
        assert not occ0.any() and seen0 == 0
        for bad_count in (0, -1):
            assert lib.zfft_detect(P, ptr(rows), bad_count, ptr(fl), ptr(fo), ptr(ev)) == _lib.ZFFT_EINVAL
        assert lib.zfft_detect(P, None, 9, ptr(fl), ptr(fo), ptr(ev)) == _lib.ZFFT_EINVAL
        with pytest.raises(ValueError):
            plan.detect(rows[:, :40])  # neither n_win nor row_length wide
        dr.assert_same(plan.detect(rows), dr.ref_detect(rows, W, 0.5, 12.0, 1, 8))
        plan.set_detect(max_per_row=0)  # off again
        assert every_call() == [_lib.ZFFT_EINVAL] * 5
    # the facade: lazily built for the first rows' width, an odd width keeps every column
    det = panadapter.Detector(threshold_db=12.0, max_per_row=4)
    with pytest.raises(AttributeError):
        det.occupancy()
    odd = rows[:, :51]
    want = dr.ref_detect(odd, 51, 0.5, 12.0, 1, 4)
    dr.assert_same(det.update(odd), want)
    dr.assert_same(det.update(odd[0]), tuple(a[:1] for a in want[:3]))
    occ = det.occupancy()
    assert occ.shape == (51,) and occ.dtype == np.float64 and det.rows_seen == 10
    np.testing.assert_array_equal(occ, (want[3] + dr.ref_detect(odd[:1], 51, 0.5, 12.0, 1, 4)[3]) / 10.0)
    det.reset()
    assert not det.occupancy().any() and det.rows_seen == 0
    det.update(rows)  # a new width rebuilds the plan
    assert det.occupancy().shape == (W,) and det.rows_seen == 9
    det.close()
