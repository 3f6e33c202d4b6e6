"""Deterministic ordering tests: plan calls enqueued behind a stalled stream.

A race test that sometimes fails is worth little.  `hold(stream, ms)` puts one bounded spin kernel
in front of the plan's work on stream A, so that everything the plan enqueues on A stays pending
while the host issues the rest of a sequence on other streams.  A call on stream B that lacks its
wait on the plan's `done_ev` then runs before its producer and reads rows that still hold the
sentinel: a reproducible wrong answer, not a flake.

`enqueue_twice` runs one sequence two ways on two fresh plans: "stepped" (a device-wide wait after
every call: the answer) and "held" (behind the hold, no wait anywhere).  The hold's length comes
from the host time the stepped pass took to enqueue: max(100 ms, 5 x that), at most 400 ms.  A
hold that ran out before the last enqueue returned is a failure ("hold too short"), never a pass.

Used by test_gpu_ordering.py; what it measured is kept in profiles/ordering/ordering.json (written
when $ZFFT_ORDERING_RECORD names a file)."""
import ctypes
import json
import os
import time

import numpy as np
import pytest

SENTINEL = 7.0          # what every buffer the plan writes holds before the hold starts
ORDER_SLEEP_S = 0.020   # the host's pause before the order events are looked at
HOLD_MIN_MS, HOLD_MAX_MS = 100.0, 400.0
NO_STREAM = "no candidate stream runs ahead of the held stream"
RECORD = {"calibration": None, "tests": {}, "cross_stream_skips": 0}

_CAL = {}
_KEEP = []      # candidate streams stay alive: a stream's hardware queue is its for life
_STREAMS = {}


def calibration():
    """{"method", "per_ms"}: spin cycles of torch.cuda._sleep per millisecond, timed once per
    session with events on a fixed count (no clock rate is assumed); a chain of matmuls (launches
    per millisecond) where _sleep is unusable."""
    if _CAL:
        return _CAL
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cycles = 2_000_000
    try:
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if not ms > 0.05:
            raise RuntimeError(f"torch.cuda._sleep({cycles}) took {ms} ms")
        _CAL.update(method="sleep", count=cycles, ms=ms, per_ms=cycles / ms)
    except (AttributeError, RuntimeError):
        m = torch.ones((4096, 4096), device="cuda")
        out = torch.empty_like(m)
        torch.matmul(m, m, out=out)
        torch.cuda.synchronize()
        a.record()
        for _ in range(8):
            torch.matmul(m, m, out=out)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        _CAL.update(method="matmul", count=8, ms=ms, per_ms=8 / ms, m=m, out=out)
    RECORD["calibration"] = {k: v for k, v in _CAL.items() if k not in ("m", "out")}
    return _CAL


def hold(stream, ms):
    """Occupies `stream` for about `ms` with bounded device work (one spin kernel of a fixed cycle
    count); returns an event recorded behind it."""
    import torch
    cal = calibration()
    ms = min(float(ms), HOLD_MAX_MS)
    with torch.cuda.stream(stream):
        if cal["method"] == "sleep":
            torch.cuda._sleep(int(ms * cal["per_ms"]))
        else:
            for _ in range(max(1, int(ms * cal["per_ms"]))):
                torch.matmul(cal["m"], cal["m"], out=cal["out"])
    ev = torch.cuda.Event()
    ev.record(stream)
    return ev


def still_held(ev):
    return not ev.query()


def stream_that_runs_ahead(held_stream, held_ev, candidates=8):
    """The first of `candidates` new streams on which a one-element fill completes while held_ev
    has not, or None.  A stream that shares the held stream's hardware queue is serialised behind
    it and would mask a missing wait."""
    import torch
    probe = torch.empty(candidates, device="cuda")
    for k in range(candidates):
        s = torch.cuda.Stream()
        _KEEP.append(s)
        with torch.cuda.stream(s):
            probe[k:k + 1].fill_(1.0)
        ev = torch.cuda.Event()
        ev.record(s)
        end = time.perf_counter() + 0.010
        while time.perf_counter() < end and not ev.query():
            pass
        if not still_held(held_ev):
            return None
        if ev.query():
            return s
    return None


def streams(null_first=False):
    """[A, B, C] for the session: A the stream to hold (HIP's NULL stream with null_first), B and C
    two streams that run ahead of it; pytest.skip with NO_STREAM when there are none."""
    import torch
    if null_first not in _STREAMS:
        a = torch.cuda.default_stream() if null_first else torch.cuda.Stream()
        _KEEP.append(a)
        torch.cuda.synchronize()
        ev = hold(a, 300.0)
        got = [a]
        for _ in range(2):
            got.append(stream_that_runs_ahead(a, ev))
        torch.cuda.synchronize()
        _STREAMS[null_first] = got
    got = _STREAMS[null_first]
    if any(s is None for s in got):
        RECORD["cross_stream_skips"] += 1
        pytest.skip(NO_STREAM)
    return got


def quiesce_count(plan):
    hook = plan.lib.zfft__plan_quiesce_count
    hook.argtypes, hook.restype = [ctypes.c_void_p], ctypes.c_int64
    return int(hook(plan._plan))


def sentinel(shape, dtype=None):
    """A device buffer the plan will write, holding defined data (never torch.empty)."""
    import torch
    return torch.full(shape, SENTINEL, device="cuda", dtype=dtype or torch.float32)


class Run:
    """One pass of a sequence: `call` for the *_device entry points, `host` for setters and
    synchronous readers.  Stepped: a device-wide wait after each.  Held: none, and an event on the
    call's stream for the order assertion."""

    def __init__(self, plan, streams_, held):
        self.plan, self.streams, self.held = plan, streams_, held
        self.hold_ev = None
        self.enqueue_s = 0.0
        self.order = []
        self.waits = {}
        self.wait_expected = False
        self.q0 = 0

    def _after(self, t0):
        import torch
        self.enqueue_s += time.perf_counter() - t0
        if not self.held:
            torch.cuda.synchronize()

    def call(self, what, fn, *args, on, **kw):
        """fn(*args, stream=<on>): a plan call enqueued on torch stream `on`."""
        import torch
        t0 = time.perf_counter()
        fn(*args, stream=on.cuda_stream, **kw)
        self._after(t0)
        if self.held:
            ev = torch.cuda.Event()
            ev.record(on)
            self.order.append((what, on, ev))

    def host(self, fn, *args, **kw):
        t0 = time.perf_counter()
        out = fn(*args, **kw)
        self._after(t0)
        return out

    def assert_held(self, when):
        if self.held:
            assert still_held(self.hold_ev), f"hold too short: it ran out before {when}"

    def expect_wait(self, when):
        """From here on a call may wait on the host (growth, a setter, a synchronous reader): the
        hold must still be in flight now, and is not asked for at the end."""
        if not self.wait_expected:
            self.assert_held(when)
        self.wait_expected = True

    def waiting(self, what, fn, *args, on=None, **kw):
        """A call that may wait on the host (on stream `on`, or a setter): whether it returned with
        the hold in flight and how many quiesces it made are recorded, not asserted."""
        import torch
        self.expect_wait(what)
        q = quiesce_count(self.plan)
        t0 = time.perf_counter()
        if on is not None:
            kw["stream"] = on.cuda_stream
        out = fn(*args, **kw)
        ms = (time.perf_counter() - t0) * 1e3
        if self.held:
            self.waits[what] = {"returned_while_held": bool(still_held(self.hold_ev)), "host_ms": round(ms, 3),
                                "quiesce_delta": quiesce_count(self.plan) - q}
            if on is not None:
                ev = torch.cuda.Event()
                ev.record(on)
                self.order.append((what, on, ev))
        self._after(t0)
        return out

    def check_order(self, skip=()):
        """Order: after the host has paused 20 ms, no event recorded behind a plan call has
        completed while the hold has not.  (On stream A that is certain; on B and C it is the
        plan's wait on done_ev.)  One pause serves every event recorded so far."""
        self.enqueue_s += ORDER_SLEEP_S
        if not self.held:
            return
        time.sleep(ORDER_SLEEP_S)
        early = [what for what, on, ev in self.order if what not in skip and ev.query()]
        assert still_held(self.hold_ev), "hold too short: it ran out during the order check"
        assert not early, f"ran ahead of the held producer: {early}"


def _host(v):
    import torch
    if isinstance(v, torch.Tensor):
        return v.cpu().numpy()
    if isinstance(v, dict):
        return {k: _host(x) for k, x in v.items()}
    if isinstance(v, (tuple, list)):
        return tuple(_host(x) for x in v)
    return v


def enqueue_twice(name, make_plan, sequence, streams_, hold_on=0):
    """make_plan() -> (plan, bufs): a fresh, warmed plan and its device buffers (inputs uploaded,
    outputs holding the sentinel).  sequence(plan, run, bufs) -> outputs (tensors, arrays, nested).
    Runs it stepped, then held behind a hold on streams_[hold_on]; returns (held, stepped, run)
    with the outputs as numpy and `run` the held pass (final_held, quiesce_delta, waits)."""
    import torch
    plan, bufs = make_plan()
    try:
        torch.cuda.synchronize()
        step = Run(plan, streams_, held=False)
        stepped = sequence(plan, step, bufs)
        torch.cuda.synchronize()
        stepped = _host(stepped)
    finally:
        plan.close()
    enqueue_ms = step.enqueue_s * 1e3
    hold_ms = min(HOLD_MAX_MS, max(HOLD_MIN_MS, 5.0 * enqueue_ms))
    plan, bufs = make_plan()
    run = Run(plan, streams_, held=True)
    try:
        torch.cuda.synchronize()
        run.q0 = quiesce_count(plan)
        run.hold_ev = hold(streams_[hold_on], hold_ms)
        try:
            held = sequence(plan, run, bufs)
            run.final_held = bool(still_held(run.hold_ev))
            run.quiesce_delta = quiesce_count(plan) - run.q0
        finally:
            torch.cuda.synchronize()
        held = _host(held)
    finally:
        plan.close()
    RECORD["tests"][name] = {"stepped_enqueue_ms": round(enqueue_ms, 3), "hold_ms": round(hold_ms, 1),
                             "held_enqueue_ms": round(run.enqueue_s * 1e3, 3),
                             "hold_in_flight_after_last_call": run.final_held,
                             "quiesce_delta": run.quiesce_delta, "host_waits": run.waits}
    if not run.wait_expected:
        assert run.final_held, f"hold too short: {hold_ms:.0f} ms ran out before the last enqueue returned"
    return held, stepped, run


def write_record():
    path = os.environ.get("ZFFT_ORDERING_RECORD")
    if path:
        with open(path, "w") as fh:
            json.dump(RECORD, fh, indent=1, sort_keys=True)


def same_bytes(held, stepped, what=""):
    """Held outputs equal stepped outputs bytewise, leaf by leaf."""
    if isinstance(stepped, dict):
        assert held.keys() == stepped.keys(), what
        for k in stepped:
            same_bytes(held[k], stepped[k], f"{what}/{k}")
    elif isinstance(stepped, tuple):
        assert len(held) == len(stepped), what
        for i, (h, s) in enumerate(zip(held, stepped)):
            same_bytes(h, s, f"{what}[{i}]")
    elif isinstance(stepped, np.ndarray):
        assert held.shape == stepped.shape and held.dtype == stepped.dtype, what
        if held.tobytes() != stepped.tobytes():
            bad = np.flatnonzero(held.reshape(-1).view(np.uint8) != stepped.reshape(-1).view(np.uint8))
            raise AssertionError(f"{what}: held differs from stepped in {bad.size} of {held.nbytes} bytes "
                                 f"(first at byte {int(bad[0])})")
    else:
        assert held == stepped, (what, held, stepped)
