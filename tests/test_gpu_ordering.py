"""The plan's asynchronous contract (include/zfft.h: every *_device entry point is "enqueued on
hip_stream; returns without syncing"), checked deterministically: the sequence under test is
enqueued behind a bounded spin kernel that holds the first stream (tests/stall.py), so a call on
another stream that lacks its wait on the plan's done_ev runs before its producer and reads rows
that still hold the sentinel 7.0.

Three kinds of assertion:
  order    an event recorded behind a plan call on B or C, whose plan-side predecessor sits behind
           the hold on A, has not completed 20 ms later while the hold has not;
  data     the held outputs equal the stepped outputs (a device-wide wait after every call)
           bytewise, and the stepped outputs meet the references the numeric tests use: the float64
           oracle through the row gate, and the bit-exact numpy rules of persistence_ref,
           detect_ref, detect_local_ref, viewport_ref, history_ref and oracle/render.py;
  no wait  after a warm pass of the same shapes the held sequence leaves the plan's quiesce count
           unchanged and the hold is still in flight when the last call has returned.
Where a host wait is expected (a workspace grows, a setter, a synchronous reader) the hold is
asserted to be in flight just before the first such call instead, and what the call did is recorded
(profiles/ordering/ordering.json).  A hold that ran out is a failure, never a pass.

COVERED maps every entry point with a `void *hip_stream` parameter to the scenarios that call it;
test_ordering_host.py holds the header against it."""
import functools

import numpy as np
import pytest

import detect_local_ref as dl
import detect_ref as dr
import history_ref as hr
import persistence_ref as pr
import stall
import viewport_ref as vr
import welch_average_ref as war
import welch_lines_ref as wl
from conftest import assert_row_close
from oracle import render as rr

pytestmark = pytest.mark.gpu
FS = 2.4e6

COVERED = {
    "zfft_process_device": ["a", "b", "c", "e_lo", "e_average", "f"],
    "zfft_waterfall_push_device": ["a", "d", "e_waterfall_reset", "f"],
    "zfft_waterfall_render_device": ["a", "d"],
    "zfft_persistence_push_device": ["a", "e_reset", "e_decay", "f"],
    "zfft_detect_device": ["a", "e_reset"],
    "zfft_detect_floors_device": ["a"],
    "zfft_viewport_push_device": ["a", "d", "e_reset", "e_hold_reset"],
    "zfft_viewport_render_device": ["a", "d"],
    "zfft_history_push_device": ["a", "e_reset"],
    "zfft_history_read_device": ["a"],
    "zfft_history_view_device": ["a"],
}


@pytest.fixture(scope="module", autouse=True)
def _gpu(zfft_lib):
    from pypanadapter_amd import device_count
    assert device_count() >= 1, "GPU tests need a HIP device"
    yield
    stall.write_record()


def _dev(a):
    import torch
    a = np.array(a, order="C")   # a copy: the cached inputs are read-only
    if np.iscomplexobj(a):
        a = a.view(np.float32)
    return torch.from_numpy(a).to("cuda")


def _frames(F, L, N, z, W, seed0, f_lo=None):
    from pypanadapter_amd import synth
    return np.stack([synth.make_iq(L, FS, seed0 + f, n_fft=N, zoom=z, n_win=W,
                                   f_lo=1.0 if f_lo is None else f_lo[f]) for f in range(F)])


def _cu8(x):
    """(uint8 interleaved I,Q as the plan takes it, the complex values those bytes mean)."""
    iq = np.ascontiguousarray(x).view(np.float32).astype(np.float64)
    b = np.clip(np.rint(127.5 + 127.5 * 0.25 * iq), 0, 255).astype(np.uint8)
    v = b.astype(np.float64) / 127.5 - 1.0
    return b, v[..., 0::2] + 1j * v[..., 1::2]


def _cycle(streams, start=1):
    """B, C, A, B, ...: every call on another stream than the call before it."""
    k = start
    while True:
        yield streams[k % 3]
        k += 1


def _view_render_ref(img, cmap, levels):
    ref = rr.render(np.nan_to_num(img.astype(np.float64), nan=0.0), rr.lookup_table(cmap), levels)
    ref[np.isnan(img)] = (*rr.lookup_table(cmap)[0][:3], 0)
    return ref


def _same_f32(got, ref, what=""):
    np.testing.assert_array_equal(np.asarray(got), np.asarray(ref, dtype=np.float32), err_msg=what)


# ---------------------------------------------------------------- a / f. producer to every consumer
A_SHAPE = dict(N=512, zoom=2, W=256, L=8192, F=2, g=1)   # 30 rows: test_gpu_detect's device case
A_DET = dict(q=0.5, thr=12.0, mw=2, K=8)
A_PERSIST = (96, -200.0, -8.0)
A_VIEW = dict(height=8, geo=(0, 256, 64), det="max", m=2)
A_HIST = dict(cap=64, lo=-150.0, hi=-50.0, lines=7, m=4)
A_LOCAL = (16, 2)


@functools.lru_cache(maxsize=None)
def _a_input():
    s = A_SHAPE
    x = war.burst_frames(s["F"], s["L"], s["N"], s["zoom"], s["W"], 9100)
    x.setflags(write=False)
    return x


def _a_bufs(count, first_only):
    import torch
    s, W, K = A_SHAPE, A_SHAPE["W"], A_DET["K"]
    b = {"x": _dev(_a_input()).reshape(s["F"], s["L"], 2), "rows": stall.sentinel((count, W))}
    b["floor"] = stall.sentinel((count,))
    b["found"] = stall.sentinel((count,), torch.int32)
    b["events"] = stall.sentinel((count, K, 4), torch.int32)
    if not first_only:
        H = W // 4
        b["floors"] = stall.sentinel((count, W))
        b["wrgba"] = stall.sentinel((H, W, 4), torch.uint8)
        b["vrgba"] = stall.sentinel((A_VIEW["height"], A_VIEW["geo"][2], 4), torch.uint8)
        b["back"] = stall.sentinel((count, W))
        b["himg"] = stall.sentinel((A_HIST["lines"], A_VIEW["geo"][2]))
    return b


def _a_sequence(local, first_only):
    s, count = A_SHAPE, 30

    def sequence(plan, run, b):
        nxt = _cycle(run.streams)
        rows = b["rows"].data_ptr()
        run.call("process", plan.process_device, b["x"].data_ptr(), s["L"], s["F"], rows, on=run.streams[0])
        run.call("waterfall_push", plan.waterfall_push_device, rows, count, on=next(nxt))
        run.call("persistence_push", plan.persistence_push_device, rows, count, on=next(nxt))
        run.call("detect", plan.detect_device, rows, count, b["floor"].data_ptr(), b["found"].data_ptr(),
                 b["events"].data_ptr(), on=next(nxt))
        out = {"rows": b["rows"], "detect": (b["floor"], b["found"], b["events"])}
        if not first_only:
            if local:
                run.call("detect_floors", plan.detect_floors_device, rows, count, b["floors"].data_ptr(), on=next(nxt))
                out["floors"] = b["floors"]
            run.call("viewport_push", plan.viewport_push_device, rows, count, on=next(nxt))
            run.call("viewport_render", plan.viewport_render_device, b["vrgba"].data_ptr(), on=next(nxt))
            run.call("history_push", plan.history_push_device, rows, count, on=next(nxt))
            run.call("history_read", plan.history_read_device, 0, count, b["back"].data_ptr(), on=next(nxt))
            g = A_VIEW["geo"]
            run.call("history_view", plan.history_view_device, b["himg"].data_ptr(), 0, A_HIST["lines"], g[2],
                     A_HIST["m"], "max", g[0], g[1], on=next(nxt))
            run.call("waterfall_render", plan.waterfall_render_device, b["wrgba"].data_ptr(), on=next(nxt))
            out.update(vrgba=b["vrgba"], back=b["back"], himg=b["himg"], wrgba=b["wrgba"])
        run.check_order()
        # synchronous readers, issued while the hold is in flight: they may block, and must
        # return what the stepped pass returns
        run.expect_wait("the synchronous readers")
        out["hist"] = run.host(plan.persistence)
        out["occ"] = run.host(plan.detect_occupancy)
        if not first_only:
            out["vimg"] = run.host(plan.viewport_image)
            out["traces"] = run.host(plan.viewport_traces)
            out["hrows"] = run.host(plan.history_rows, 0, count)
        out["wimg"] = run.host(plan.waterfall_image)
        out["levels_before"] = plan.waterfall_levels()
        if not first_only:
            out["auto"] = run.host(plan.waterfall_autolevel)
        return out
    return sequence


def _a_make_plan(local, fmt, first_only, streams):
    from pypanadapter_amd import ZoomFFT
    s = A_SHAPE
    seq = _a_sequence(local, first_only)

    def make():
        plan = ZoomFFT(s["N"], s["zoom"], FS, n_win=s["W"], segments_per_line=s["g"])
        assert plan.lines(s["L"]) * s["F"] == 30
        plan.set_persistence(*A_PERSIST)
        plan.set_detect(A_DET["q"], A_DET["thr"], A_DET["mw"], A_DET["K"])
        if local:
            plan.set_detect_local(*A_LOCAL)
        if not first_only:
            v = A_VIEW
            plan.set_viewport(v["height"], v["geo"][2], v["geo"][0], v["geo"][1], v["det"], v["m"])
            plan.set_history(A_HIST["cap"], fmt, A_HIST["lo"], A_HIST["hi"])
        # warm pass of the same shapes (every workspace, table and scratch is sized), then the
        # state back to that of a fresh plan
        levels = plan.waterfall_levels()
        seq(plan, stall.Run(plan, streams, held=False), _a_bufs(30, first_only))
        plan.persistence_reset()
        plan.detect_reset()
        if not first_only:
            plan.viewport_reset()
            plan.history_reset()
        plan.waterfall_reset(1)
        plan.waterfall_levels(*levels)
        return plan, _a_bufs(30, first_only)
    return make


def _a_check(held, stepped, local, fmt, first_only):
    from pypanadapter_amd.engine import EMISSION_DTYPE
    s, W, x = A_SHAPE, A_SHAPE["W"], _a_input()
    stall.same_bytes(held, stepped, "held")
    rows = stepped["rows"]
    for f in range(s["F"]):
        ref = wl.ref_lines(x[f], FS, s["N"], s["zoom"], W, s["g"], "mean")
        for r in range(15):
            assert_row_close(rows[f * 15 + r], ref[r], f"frame {f} line {r}")
    d = A_DET
    got = (stepped["detect"][0], stepped["detect"][1],
           np.ascontiguousarray(stepped["detect"][2]).view(EMISSION_DTYPE).reshape(30, d["K"]))
    if local:
        want = dl.ref_detect_local(rows, W, A_LOCAL[0], A_LOCAL[1], d["q"], d["thr"], d["mw"], d["K"])
    else:
        want = dr.ref_detect(rows, W, d["q"], d["thr"], d["mw"], d["K"])
    assert want[3].any() and (local or want[1].sum() >= 30)   # the in-band tones of the golden recipe
    dr.assert_same(got, want)
    np.testing.assert_array_equal(stepped["occ"][0], want[3])
    assert stepped["occ"][1] == 30
    np.testing.assert_array_equal(stepped["hist"][0], pr.ref_hist(rows, *A_PERSIST, W))
    assert stepped["hist"][1] == 30
    lut = rr.lookup_table("Default")
    assert not (stepped["wimg"] == stall.SENTINEL).any(), "a sentinel row reached the ring"
    if first_only:
        return
    if local:
        dl.assert_floors_same(stepped["floors"], dl.ref_local_floors(rows, W, A_LOCAL[0], A_LOCAL[1], d["q"]), W)
    v = A_VIEW
    lines, pend = vr.ref_lines(rows, W, v["geo"], v["det"], v["m"])
    assert len(lines) == 15 and pend[0] == 0
    _same_f32(stepped["vimg"], vr.ref_image(lines, v["height"], 1), "viewport image")
    for got_t, ref_t, name in zip(stepped["traces"], vr.ref_holds(lines), ("last", "max_hold", "min_hold")):
        _same_f32(got_t, ref_t, name)
    h = A_HIST
    kept = hr.stored(rows, fmt, h["lo"], h["hi"])
    for key in ("back", "hrows"):
        g, k = stepped[key], kept
        np.testing.assert_array_equal(np.isnan(g), np.isnan(k), err_msg=key)
        np.testing.assert_array_equal(g[~np.isnan(k)].view(np.uint32), k[~np.isnan(k)].view(np.uint32), err_msg=key)
    _same_f32(stepped["himg"], hr.ref_view(kept, 0, W, 0, h["lines"], v["geo"], "max", h["m"]), "history view")
    np.testing.assert_array_equal(stepped["wrgba"], rr.render(stepped["wimg"].astype(np.float64), lut,
                                                              stepped["levels_before"]))
    np.testing.assert_array_equal(stepped["vrgba"], _view_render_ref(stepped["vimg"], "Default",
                                                                     stepped["levels_before"]))
    assert stepped["auto"] == rr.autolevel(stepped["wimg"].astype(np.float64))


@pytest.mark.parametrize("local,fmt", [(False, "u8"), (True, "f32")], ids=["global_u8", "local_f32"])
def test_a_producer_to_every_consumer(local, fmt):
    """process_device on held A, then every consumer on another stream than the call before it
    (B, C, A, B, ...): order and data on every call, then the synchronous readers while held."""
    streams = stall.streams()
    name = f"a[{'local' if local else 'global'}_{fmt}]"
    held, stepped, run = stall.enqueue_twice(name, _a_make_plan(local, fmt, False, streams),
                                             _a_sequence(local, False), streams)
    _a_check(held, stepped, local, fmt, False)


def test_f_the_null_stream():
    """Scenario a's first three steps (and the global detector) with HIP's NULL stream as the held
    stream A and torch streams as B and C."""
    streams = stall.streams(null_first=True)
    assert streams[0].cuda_stream == 0
    held, stepped, run = stall.enqueue_twice("f", _a_make_plan(False, "u8", True, streams),
                                             _a_sequence(False, True), streams)
    _a_check(held, stepped, False, "u8", True)


# ---------------------------------------------------------------- b. process_device chains
# N 1024, F 2, L about 20000 (every decimator's domain starts at or below 16384 samples).  Path 2
# needs eight edge windows of 8192 samples: the nearest shape inside its domain is L = 65536 + k.
B_CASES = {
    "z8_path1": dict(N=1024, zoom=8, path=1), "z8_path2": dict(N=1024, zoom=8, path=2, L0=65536),
    "z8_path3": dict(N=1024, zoom=8, path=3), "z8_path4": dict(N=1024, zoom=8, path=4),
    "z8_path5": dict(N=1024, zoom=8, path=5), "z8_path6": dict(N=1024, zoom=8, path=6),
    "z4_path5": dict(N=1024, zoom=4, path=5), "z4_path6": dict(N=1024, zoom=4, path=6),
    "z2_path4": dict(N=1024, zoom=2, path=4), "z2_path7": dict(N=1024, zoom=2, path=7),
    "z16_path6_fc_head_xa_tail": dict(N=1024, zoom=16, path=6),
    "z1_cu8_ingest": dict(N=1024, zoom=1, in_dtype="cu8"),
    "welch_four_step": dict(N=4096, zoom=2, welch=2),
    "median_wsegs": dict(N=1024, zoom=8, average="median"),
}
B_OFFSETS = (3, 6, 1, 4, 7)   # L mod 8 of the five calls; the warm pass runs at the largest
B_W, B_F = 128, 2
GATE_MS = 50.0


def _plan_of(c, **kw):
    from pypanadapter_amd import ZoomFFT
    plan = ZoomFFT(c["N"], c["zoom"], FS, n_win=B_W, in_dtype=c.get("in_dtype", "complex64"),
                   average=c.get("average", "mean"), **kw)
    if c.get("path"):
        plan.set_path(c["path"])
    if c.get("welch"):
        plan.set_welch(c["welch"])
    return plan


@functools.lru_cache(maxsize=None)
def _case_frames(name, L, F, seed0):
    """(what the plan takes, the complex values it means) for F frames of length L; beyond three
    frames the same three in turn (a 70-frame call is about where its frames go, not what they hold)."""
    c = {**B_CASES, **C_CASES}[name]
    x = _frames(min(F, 3), L, c["N"], c["zoom"], B_W, seed0)
    x = x[np.arange(F) % 3] if F > 3 else x
    arr, vals = _cu8(x) if c.get("in_dtype") == "cu8" else (x, x)
    return arr, vals


def _oracle_rows(oracle_lib, c, vals, rows, what, frames=None, f_lo=None):
    for f in (range(len(vals)) if frames is None else frames):
        if c.get("average", "mean") == "mean":
            ref = oracle_lib.psd_row(vals[f], FS, c["N"], c["zoom"], B_W, f_lo=1.0 if f_lo is None else f_lo[f])
        else:
            ref = war.ref_row(vals[f], FS, c["N"], c["zoom"], B_W, c["average"])
        assert_row_close(rows[f], ref, f"{what} frame {f}")


@pytest.mark.parametrize("name", list(B_CASES))
def test_b_process_chain(oracle_lib, name):
    """Five process_device calls in steady state, inputs and L mod 8 differing: A, A, B -- order for
    the third -- then B again behind a gate (B waits for the hold's end, then spins 50 ms more) and
    back on A.  The last call's wait on done_ev, recorded on B, is the A -> B -> A chain: its end
    event must not precede the gate's.  No host wait anywhere: the quiesce count stays and the hold
    is in flight when the last call has returned."""
    import torch
    c = B_CASES[name]
    Ls = [c.get("L0", 20000) + k for k in B_OFFSETS]
    streams = stall.streams()
    A, B = streams[0], streams[1]
    data = [_case_frames(name, L, B_F, 7000 + L) for L in Ls]
    t = {}

    def make():
        plan = _plan_of(c)
        Lmax = max(Ls)
        warm = _dev(_case_frames(name, Lmax, B_F, 7000 + Lmax)[0])
        wrows = stall.sentinel((B_F, B_W))
        plan.process_device(warm.data_ptr(), Lmax, B_F, wrows.data_ptr(), A.cuda_stream)
        torch.cuda.synchronize()
        return plan, {"x": [_dev(d[0]) for d in data], "rows": [stall.sentinel((B_F, B_W)) for _ in Ls]}

    def sequence(plan, run, b):
        def go(k, on):
            run.call(f"process{k + 1}", plan.process_device, b["x"][k].data_ptr(), Ls[k], B_F,
                     b["rows"][k].data_ptr(), on=on)
        go(0, A)
        go(1, A)
        go(2, B)
        run.check_order()
        if run.held:   # the gate: B waits for the hold's end, then spins GATE_MS more
            B.wait_event(run.hold_ev)
            stall.hold(B, GATE_MS)
            t["gate"] = torch.cuda.Event(enable_timing=True)
            t["gate"].record(B)
        go(3, B)
        go(4, A)
        if run.held:
            t["last"] = torch.cuda.Event(enable_timing=True)
            t["last"].record(A)
        return {"rows": b["rows"]}

    held, stepped, run = stall.enqueue_twice(f"b[{name}]", make, sequence, streams)
    assert run.quiesce_delta == 0, f"the plan waited on the host {run.quiesce_delta} times in steady state"
    assert run.final_held
    after = t["gate"].elapsed_time(t["last"])
    print(f"b[{name}]: the call back on A ended {after:.3f} ms after B's gate")
    assert after > 0.0, f"the call back on A ended {-after:.3f} ms before B's gate: it did not wait for B's call"
    stall.same_bytes(held, stepped, "held")
    for k, L in enumerate(Ls):
        _oracle_rows(oracle_lib, c, data[k][1], stepped["rows"][k], f"call {k + 1} L={L}")


# ---------------------------------------------------------------- c. growth behind the hold
# Warm with one frame at the shorter length; behind the hold one frame, then a call that needs
# larger workspaces (more frames at the same length, so that no LO rebuild waits first), then one
# frame on B.  `big`: (L, F) of the larger call.
C_CASES = {
    "growth_yf_ping_pong_path1": dict(N=1024, zoom=8, path=1, L=20003, big=(20003, 70)),   # crosses a 64-frame group
    "growth_xa_path3": dict(N=1024, zoom=8, path=3, L=20003, big=(20003, 3)),
    "growth_pc_path4": dict(N=1024, zoom=8, path=4, L=20003, big=(20003, 3)),
    "growth_fc_edge_v_path6": dict(N=1024, zoom=8, path=6, L=20003, big=(20003, 3)),
    "growth_dec_cu8": dict(N=1024, zoom=1, in_dtype="cu8", L=20003, big=(20003, 3)),
    "growth_wparts": dict(N=1024, zoom=8, L=24579, big=(24579, 3)),            # 5 segments: the split form
    "growth_means_z4": dict(N=4096, zoom=2, welch=2, L=20003, big=(20003, 3)),
    "growth_wsegs": dict(N=1024, zoom=8, average="median", L=20003, big=(20003, 3)),
    "growth_ensure_window": dict(N=1024, zoom=8, L=20003, big=(4099, 1)),      # L_d = 513 < n_fft: a new window
    "growth_ensure_lo": dict(N=1024, zoom=8, L=20003, big=(40006, 1)),         # a longer LO row
}


@pytest.mark.parametrize("name", list(C_CASES))
def test_c_growth(oracle_lib, name):
    """Data only: whatever the larger call does about the work enqueued before it (DevBuf::ensure
    frees and allocates; hipFree waits for the device), all three calls give the stepped rows.
    Whether it returned with the hold in flight, and its quiesces, are recorded."""
    import torch
    c = C_CASES[name]
    L, (Lb, Fb) = c["L"], c["big"]
    streams = stall.streams()
    A, B = streams[0], streams[1]
    shapes = [(L, 1, 8100), (Lb, Fb, 8200), (L, 1, 8300)]
    data = [_case_frames(name, l, f, seed) for l, f, seed in shapes]

    def make():
        plan = _plan_of(c)
        warm = _dev(_case_frames(name, L, 1, 8000)[0])
        wrows = stall.sentinel((1, B_W))
        plan.process_device(warm.data_ptr(), L, 1, wrows.data_ptr(), A.cuda_stream)
        torch.cuda.synchronize()
        return plan, {"x": [_dev(d[0]) for d in data], "rows": [stall.sentinel((f, B_W)) for _, f, _ in shapes]}

    def sequence(plan, run, b):
        args = [(b["x"][k].data_ptr(), shapes[k][0], shapes[k][1], b["rows"][k].data_ptr()) for k in range(3)]
        run.call("process1", plan.process_device, *args[0], on=A)
        run.waiting("larger call", plan.process_device, *args[1], on=A)
        run.call("process3", plan.process_device, *args[2], on=B)
        return {"rows": b["rows"]}

    held, stepped, run = stall.enqueue_twice(f"c[{name}]", make, sequence, streams)
    print(f"c[{name}]: {run.waits}")
    stall.same_bytes(held, stepped, "held")
    for k, (l, f, _) in enumerate(shapes):
        frames = None if f <= 3 else (0, 1, 63, 64, f - 1)
        _oracle_rows(oracle_lib, c, data[k][1], stepped["rows"][k], f"call {k + 1} L={l}", frames)


# ---------------------------------------------------------------- d. colormap change between renders
D_W, D_ROWS, D_VIEW = 256, 20, (8, 64)


@functools.lru_cache(maxsize=None)
def _level_rows(count, W, seed):
    """Seeded rows around -170 with two planted emissions (columns 40..43 and 100..102)."""
    rng = np.random.default_rng(seed)
    rows = (-170.0 + 15.0 * rng.standard_normal((count, W))).astype(np.float32)
    rows[:, 40:44] = -130.0 + rng.random((count, 4)).astype(np.float32)
    rows[:, 100:103] = -125.0 + rng.random((count, 3)).astype(np.float32)
    rows.setflags(write=False)
    return rows


@pytest.mark.parametrize("warm_luts", [False, True], ids=["first_uploads", "warmed_uploads"])
def test_d_colormap_change_between_enqueued_renders(warm_luts):
    """Rows pushed on held A; colormap Tropical and a render on A; colormap Matrix and a render on
    B: the first image is Tropical's, the second Matrix's, for the ring and for the viewport.  The
    LUT is rebuilt in a plan-owned pageable array and uploaded on the render's stream: what each
    render did on the host is recorded (measured: it returns in 15 us with the hold in flight, the
    runtime having staged the table at the call), and the order of the renders on B is asserted.  `warmed_uploads` has uploaded both tables once
    before the hold, so that no first-use cost of the pageable copy hides the device-side order."""
    import torch
    from pypanadapter_amd import ZoomFFT
    streams = stall.streams()
    A, B = streams[0], streams[1]
    rows = _level_rows(D_ROWS, D_W, 31)
    H = D_W // 4

    def bufs():
        return {"rows": _dev(rows), "w1": stall.sentinel((H, D_W, 4), torch.uint8),
                "w2": stall.sentinel((H, D_W, 4), torch.uint8), "v1": stall.sentinel((*D_VIEW, 4), torch.uint8),
                "v2": stall.sentinel((*D_VIEW, 4), torch.uint8)}

    def make():
        plan = ZoomFFT(512, 2, FS, n_win=D_W)
        plan.set_viewport(D_VIEW[0], D_VIEW[1], 0, D_W, "max", 2)
        b = bufs()
        st = A.cuda_stream
        plan.waterfall_push_device(b["rows"].data_ptr(), D_ROWS, st)
        plan.viewport_push_device(b["rows"].data_ptr(), D_ROWS, st)
        for cmap in (("Tropical", "Matrix") if warm_luts else ()) + ("Default",):
            plan.waterfall_colormap(cmap)
            plan.waterfall_render_device(b["w1"].data_ptr(), st)
            plan.viewport_render_device(b["v1"].data_ptr(), st)
            torch.cuda.synchronize()
        plan.viewport_reset()
        plan.waterfall_reset(1)
        torch.cuda.synchronize()
        return plan, bufs()

    def sequence(plan, run, b):
        run.call("waterfall_push", plan.waterfall_push_device, b["rows"].data_ptr(), D_ROWS, on=A)
        run.call("viewport_push", plan.viewport_push_device, b["rows"].data_ptr(), D_ROWS, on=A)
        run.host(plan.waterfall_colormap, "Tropical")
        run.waiting("waterfall render Tropical on A", plan.waterfall_render_device, b["w1"].data_ptr(), on=A)
        run.host(plan.waterfall_colormap, "Matrix")
        run.waiting("waterfall render Matrix on B", plan.waterfall_render_device, b["w2"].data_ptr(), on=B)
        run.host(plan.waterfall_colormap, "Tropical")
        run.waiting("viewport render Tropical on A", plan.viewport_render_device, b["v1"].data_ptr(), on=A)
        run.host(plan.waterfall_colormap, "Matrix")
        run.waiting("viewport render Matrix on B", plan.viewport_render_device, b["v2"].data_ptr(), on=B)
        run.check_order()
        out = {k: b[k] for k in ("w1", "w2", "v1", "v2")}
        out["wimg"] = run.host(plan.waterfall_image)
        out["vimg"] = run.host(plan.viewport_image)
        out["levels"] = plan.waterfall_levels()
        return out

    name = f"d[{'warmed' if warm_luts else 'first'}_uploads]"
    held, stepped, run = stall.enqueue_twice(name, make, sequence, streams)
    print(f"{name}: {run.waits}")
    for cmap, w, v in (("Tropical", "w1", "v1"), ("Matrix", "w2", "v2")):
        want_w = rr.render(stepped["wimg"].astype(np.float64), rr.lookup_table(cmap), stepped["levels"])
        want_v = _view_render_ref(stepped["vimg"], cmap, stepped["levels"])
        for which, out in (("stepped", stepped), ("held", held)):
            np.testing.assert_array_equal(out[w], want_w, err_msg=f"{which} ring image, {cmap}")
            np.testing.assert_array_equal(out[v], want_v, err_msg=f"{which} viewport image, {cmap}")
    stall.same_bytes(held, stepped, "held")


# ---------------------------------------------------------------- e. setters and resets between pushes
E_W, E_N1, E_N2 = 256, 12, 10
E_PERSIST = (64, -200.0, -100.0)
E_DET = dict(q=0.5, thr=12.0, mw=2, K=8)
E_VIEW = dict(height=16, geo=(0, 256, 64), det="max", m=2)
E_HIST = dict(cap=32, fmt="u8", lo=-190.0, hi=-130.0)


def _e_plan(scroll=1):
    from pypanadapter_amd import ZoomFFT
    plan = ZoomFFT(512, 2, FS, n_win=E_W, scroll=scroll)
    plan.set_persistence(*E_PERSIST)
    plan.set_detect(E_DET["q"], E_DET["thr"], E_DET["mw"], E_DET["K"])
    v = E_VIEW
    plan.set_viewport(v["height"], v["geo"][2], v["geo"][0], v["geo"][1], v["det"], v["m"])
    plan.set_history(E_HIST["cap"], E_HIST["fmt"], E_HIST["lo"], E_HIST["hi"])
    return plan


def _e_det_bufs(count):
    import torch
    return (stall.sentinel((count,)), stall.sentinel((count,), torch.int32),
            stall.sentinel((count, E_DET["K"], 4), torch.int32))


def _e_push_all(plan, run, rows, count, det, nxt, tag):
    p = rows.data_ptr()
    run.call(f"persistence_push{tag}", plan.persistence_push_device, p, count, on=next(nxt))
    run.call(f"detect{tag}", plan.detect_device, p, count, det[0].data_ptr(), det[1].data_ptr(),
             det[2].data_ptr(), on=next(nxt))
    run.call(f"viewport_push{tag}", plan.viewport_push_device, p, count, on=next(nxt))
    run.call(f"history_push{tag}", plan.history_push_device, p, count, on=next(nxt))


def _e_make(streams, scroll=1):
    import torch
    r1, r2 = _level_rows(E_N1, E_W, 41), _level_rows(E_N2, E_W, 42)

    def bufs():
        return {"r1": _dev(r1), "r2": _dev(r2), "d1": _e_det_bufs(E_N1), "d2": _e_det_bufs(E_N2)}

    def make():
        plan = _e_plan(scroll)
        b = bufs()
        warm = stall.Run(plan, streams, held=False)
        _e_push_all(plan, warm, b["r1"], E_N1, b["d1"], _cycle(streams, 0), "")
        plan.waterfall_push_device(b["r1"].data_ptr(), E_N1, streams[0].cuda_stream)
        torch.cuda.synchronize()
        plan.persistence_reset()
        plan.detect_reset()
        plan.viewport_reset()
        plan.history_reset()
        plan.waterfall_reset(scroll)
        torch.cuda.synchronize()
        return plan, bufs()
    return make, r1, r2


def _e_state(plan, run, n_hist):
    return {"hist": run.host(plan.persistence), "occ": run.host(plan.detect_occupancy),
            "vimg": run.host(plan.viewport_image), "traces": run.host(plan.viewport_traces),
            "hstate": plan.history_state(), "hrows": run.host(plan.history_rows, plan.history_state()[1], n_hist)}


def _e_finish(run):
    """Order (none of these setters waits on the host: each enqueues on the plan's stream behind
    done_ev); then the synchronous readers may wait."""
    run.check_order()
    run.expect_wait("the synchronous readers")


def test_e_reset_between_pushes():
    """push(rows1) over the streams, the four resets, push(rows2): the state is rows2's alone."""
    streams = stall.streams()
    make, r1, r2 = _e_make(streams)

    def sequence(plan, run, b):
        nxt = _cycle(run.streams, 0)
        _e_push_all(plan, run, b["r1"], E_N1, b["d1"], nxt, "1")
        for what, fn in (("persistence_reset", plan.persistence_reset), ("detect_reset", plan.detect_reset),
                         ("viewport_reset", plan.viewport_reset), ("history_reset", plan.history_reset)):
            run.waiting(what, fn)
        _e_push_all(plan, run, b["r2"], E_N2, b["d2"], nxt, "2")
        _e_finish(run)
        return {"d1": b["d1"], "d2": b["d2"], **_e_state(plan, run, E_N2)}

    held, stepped, run = stall.enqueue_twice("e[reset]", make, sequence, streams)
    print(f"e[reset]: {run.waits}")
    stall.same_bytes(held, stepped, "held")
    from pypanadapter_amd.engine import EMISSION_DTYPE
    d, v = E_DET, E_VIEW
    for rows, key in ((r1, "d1"), (r2, "d2")):
        want = dr.ref_detect(rows, E_W, d["q"], d["thr"], d["mw"], d["K"])
        assert want[1].sum() >= len(rows)
        got = stepped[key]
        dr.assert_same((got[0], got[1], np.ascontiguousarray(got[2]).view(EMISSION_DTYPE).reshape(len(rows), d["K"])),
                       want)
    np.testing.assert_array_equal(stepped["occ"][0], want[3])
    assert stepped["occ"][1] == E_N2
    np.testing.assert_array_equal(stepped["hist"][0], pr.ref_hist(r2, *E_PERSIST, E_W))
    assert stepped["hist"][1] == E_N2
    lines, _ = vr.ref_lines(r2, E_W, v["geo"], v["det"], v["m"])
    _same_f32(stepped["vimg"], vr.ref_image(lines, v["height"], 1), "viewport image")
    for got_t, ref_t in zip(stepped["traces"], vr.ref_holds(lines)):
        _same_f32(got_t, ref_t, "trace")
    assert stepped["hstate"] == (E_N2, 0)
    _same_f32(stepped["hrows"], hr.stored(r2, E_HIST["fmt"], E_HIST["lo"], E_HIST["hi"]), "history rows")


def test_e_decay_between_pushes():
    """push, persistence_decay(0.5), push: floor(c / 2) of the first table plus the second."""
    streams = stall.streams()
    make, r1, r2 = _e_make(streams)

    def sequence(plan, run, b):
        run.call("persistence_push1", plan.persistence_push_device, b["r1"].data_ptr(), E_N1, on=run.streams[0])
        run.waiting("persistence_decay", plan.persistence_decay, 0.5)
        run.call("persistence_push2", plan.persistence_push_device, b["r2"].data_ptr(), E_N2, on=run.streams[1])
        _e_finish(run)
        return {"hist": run.host(plan.persistence)}

    held, stepped, run = stall.enqueue_twice("e[decay]", make, sequence, streams)
    print(f"e[decay]: {run.waits}")
    stall.same_bytes(held, stepped, "held")
    h1 = pr.ref_hist(r1, *E_PERSIST, E_W)
    want = np.floor(h1.astype(np.float64) * 0.5).astype(np.uint32) + pr.ref_hist(r2, *E_PERSIST, E_W)
    np.testing.assert_array_equal(stepped["hist"][0], want)
    assert stepped["hist"][1] == int(np.floor(E_N1 * 0.5)) + E_N2


def test_e_hold_reset_between_pushes():
    """viewport_hold_reset between two pushes: the image keeps every line, max and min hold those
    of the second push alone."""
    streams = stall.streams()
    make, r1, r2 = _e_make(streams)

    def sequence(plan, run, b):
        run.call("viewport_push1", plan.viewport_push_device, b["r1"].data_ptr(), E_N1, on=run.streams[0])
        run.waiting("viewport_hold_reset", plan.viewport_hold_reset)
        run.call("viewport_push2", plan.viewport_push_device, b["r2"].data_ptr(), E_N2, on=run.streams[1])
        _e_finish(run)
        return {"vimg": run.host(plan.viewport_image), "traces": run.host(plan.viewport_traces)}

    held, stepped, run = stall.enqueue_twice("e[hold_reset]", make, sequence, streams)
    print(f"e[hold_reset]: {run.waits}")
    stall.same_bytes(held, stepped, "held")
    v = E_VIEW
    l1, p1 = vr.ref_lines(r1, E_W, v["geo"], v["det"], v["m"])
    l2, p2 = vr.ref_lines(r2, E_W, v["geo"], v["det"], v["m"], p1)
    assert p1[0] == 0 and p2[0] == 0
    _same_f32(stepped["vimg"], vr.ref_image(np.concatenate([l1, l2]), v["height"], 1), "viewport image")
    for got_t, ref_t in zip(stepped["traces"], vr.ref_holds(l2)):
        _same_f32(got_t, ref_t, "trace")


def test_e_waterfall_reset_between_pushes():
    """waterfall_reset(-1) between two pushes: the ring holds the second push alone, scrolling the
    other way -- the image of a plan that was reset and then given those rows one by one."""
    streams = stall.streams()
    make, r1, r2 = _e_make(streams)

    def sequence(plan, run, b):
        run.call("waterfall_push1", plan.waterfall_push_device, b["r1"].data_ptr(), E_N1, on=run.streams[0])
        run.waiting("waterfall_reset", plan.waterfall_reset, -1)
        run.call("waterfall_push2", plan.waterfall_push_device, b["r2"].data_ptr(), E_N2, on=run.streams[1])
        _e_finish(run)
        return {"wimg": run.host(plan.waterfall_image)}

    held, stepped, run = stall.enqueue_twice("e[waterfall_reset]", make, sequence, streams)
    print(f"e[waterfall_reset]: {run.waits}")
    stall.same_bytes(held, stepped, "held")
    with _e_plan() as ref:
        ref.waterfall_reset(-1)
        for r in r2:
            ref.waterfall_push(r)
        want = ref.waterfall_image()
    np.testing.assert_array_equal(stepped["wimg"], want)


E_LO = dict(N=1024, zoom=8, L=20003, F=2)
IF_LOS = [1.0 + k * 150e3 for k in range(8)]   # config 4's IF centre frequencies (test_gpu_parity)


def test_e_lo_frames_between_process_calls(oracle_lib):
    """set_lo_frames(IF_LOS, 1) between two process_device calls: the first call's rows use the
    plan's LO, the second's the new rows, each within the oracle gate."""
    import torch
    c = E_LO
    streams = stall.streams()
    A, B = streams[0], streams[1]
    x1 = _frames(c["F"], c["L"], c["N"], c["zoom"], B_W, 9300)
    x2 = _frames(c["F"], c["L"], c["N"], c["zoom"], B_W, 9400, f_lo=IF_LOS)

    def make():
        plan = _plan_of(c)
        rows = stall.sentinel((c["F"], B_W))
        plan.set_lo_frames(IF_LOS, 1)
        plan.process_device(_dev(x2).data_ptr(), c["L"], c["F"], rows.data_ptr(), A.cuda_stream)
        torch.cuda.synchronize()
        plan.set_lo_frames([], 1)
        plan.process_device(_dev(x1).data_ptr(), c["L"], c["F"], rows.data_ptr(), A.cuda_stream)
        torch.cuda.synchronize()
        return plan, {"x1": _dev(x1), "x2": _dev(x2), "rows1": stall.sentinel((c["F"], B_W)),
                      "rows2": stall.sentinel((c["F"], B_W))}

    def sequence(plan, run, b):
        run.call("process1", plan.process_device, b["x1"].data_ptr(), c["L"], c["F"], b["rows1"].data_ptr(), on=A)
        run.waiting("set_lo_frames", plan.set_lo_frames, IF_LOS, 1)
        run.waiting("process2 (LO rebuild)", plan.process_device, b["x2"].data_ptr(), c["L"], c["F"],
                    b["rows2"].data_ptr(), on=B)
        return {"rows1": b["rows1"], "rows2": b["rows2"]}

    held, stepped, run = stall.enqueue_twice("e[lo_frames]", make, sequence, streams)
    print(f"e[lo_frames]: {run.waits}")
    stall.same_bytes(held, stepped, "held")
    _oracle_rows(oracle_lib, c, x1, stepped["rows1"], "old LO")
    _oracle_rows(oracle_lib, c, x2, stepped["rows2"], "new LO", f_lo=IF_LOS)


E_AVG = dict(N=512, zoom=2, L=8192, F=2, W=256)


def test_e_average_and_lines_between_process_calls():
    """set_average("max") and set_segments_per_line(1) between process_device calls on A, B and C:
    mean rows, max rows, then max lines.  Neither setter waits: order and no host wait as well."""
    import torch
    from pypanadapter_amd import ZoomFFT
    c = E_AVG
    streams = stall.streams()
    x = war.burst_frames(c["F"], c["L"], c["N"], c["zoom"], c["W"], 9500)
    R = 15

    def bufs():
        return {"x": _dev(x), "mean": stall.sentinel((c["F"], c["W"])), "max": stall.sentinel((c["F"], c["W"])),
                "lines": stall.sentinel((c["F"] * R, c["W"]))}

    def steps(plan, run, b):
        for key, setter in (("mean", None), ("max", lambda: plan.set_average("max")),
                            ("lines", lambda: plan.set_segments_per_line(1))):
            if setter:
                run.host(setter)
            yield key

    def sequence(plan, run, b):
        for k, key in enumerate(steps(plan, run, b)):
            run.call(f"process_{key}", plan.process_device, b["x"].data_ptr(), c["L"], c["F"], b[key].data_ptr(),
                     on=run.streams[k])
        run.check_order()
        return {k: b[k] for k in ("mean", "max", "lines")}

    def make():
        plan = ZoomFFT(c["N"], c["zoom"], FS, n_win=c["W"])
        assert plan.lines(c["L"]) == 1
        sequence(plan, stall.Run(plan, streams, held=False), bufs())
        plan.set_average("mean")
        plan.set_segments_per_line(0)
        torch.cuda.synchronize()
        return plan, bufs()

    held, stepped, run = stall.enqueue_twice("e[average]", make, sequence, streams)
    assert run.quiesce_delta == 0 and run.final_held
    stall.same_bytes(held, stepped, "held")
    for f in range(c["F"]):
        assert_row_close(stepped["mean"][f], war.ref_row(x[f], FS, c["N"], c["zoom"], c["W"], "mean"), f"mean {f}")
        assert_row_close(stepped["max"][f], war.ref_row(x[f], FS, c["N"], c["zoom"], c["W"], "max"), f"max {f}")
        ref = wl.ref_lines(x[f], FS, c["N"], c["zoom"], c["W"], 1, "max")
        assert len(ref) == R
        for r in range(R):
            assert_row_close(stepped["lines"][f * R + r], ref[r], f"max lines frame {f} line {r}")
