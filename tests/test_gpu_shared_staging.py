"""GPU check of the one hazard the shared row staging adds: persistence, the detector with a local
floor, the viewport and the history of one plan all stage their host rows (and `history_rows` its
read-back) in the same device buffer.  A plan with all four on is fed host pushes of 3, 40, 1 and
17 rows -- the staging grows, then is used well below its capacity -- every batch to every
consumer in an order that rotates from batch to batch, with a `history_rows` read between two of
the pushes.  Four plans with one consumer each get the same rows.  Everything the shared plan
returns or holds must equal, bit for bit, what the single-consumer plans give; their own suites
tie those to the references.  Switching the viewport off releases the shared staging: a push to
two of the other consumers after that must still agree."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
FS = 2.4e6
N_FFT, ZOOM, W = 1024, 8, 128
BATCHES = (3, 40, 1, 17)
TAIL = 5  # rows pushed after the viewport went off; with them the history ring (64 rows) wraps
OPS = ("persistence", "detect", "floors", "viewport", "history")
READ_AFTER = 2  # the history read goes after this many of a batch's pushes


def _rows():
    """Seeded rows over -230 .. -110 (both clamps of the history's codes, -220 and -120, are hit)
    with a few carriers 30 dB up that wander from row to row, so that the detector has runs to
    record."""
    rng = np.random.default_rng(20240611)
    n = sum(BATCHES) + TAIL
    rows = rng.uniform(-230.0, -110.0, size=(n, W)).astype(np.float32)
    for r in range(n):
        for c in (10 + r % 7, 60, 100 - r % 5):
            rows[r, c:c + 3] = -80.0 + np.float32(r % 3)
    return rows


def _enable(plan, which):
    if "persistence" in which:
        plan.set_persistence(16, -200.0, -100.0)
    if "detect" in which:
        plan.set_detect()
        plan.set_detect_local(4, 1)
    if "viewport" in which:
        plan.set_viewport(8, 32, rows_per_line=2)
    if "history" in which:
        plan.set_history(64, "u8")


def _call(plan, op, rows):
    """One host push; what it returns, as a tuple of arrays."""
    if op == "persistence":
        return plan.persistence_push(rows) or ()
    if op == "detect":
        return plan.detect(rows)
    if op == "floors":
        return (plan.detect_floors(rows),)
    if op == "viewport":
        return plan.viewport_push(rows) or ()
    return plan.history_push(rows) or ()


def _state(plan, which):
    """What the consumers `which` of a plan hold, read back: name -> tuple of arrays."""
    out = {}
    if "persistence" in which:
        out["persistence"] = plan.persistence()
    if "detect" in which:
        out["detect_occupancy"] = plan.detect_occupancy()
    if "viewport" in which:
        out["viewport_image"] = (plan.viewport_image(),)
        out["viewport_traces"] = plan.viewport_traces()
    if "history" in which:
        seen, oldest = plan.history_state()
        out["history_rows"] = (plan.history_rows(oldest, seen - oldest),)
    return out


def _same_bits(got, ref, what):
    assert len(got) == len(ref), what
    for k, (a, b) in enumerate(zip(got, ref)):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)  # (rows_seen comes as an int)
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}[{k}]"
        assert a.tobytes() == b.tobytes(), f"{what}[{k}] differs"


def test_four_consumers_behind_one_staging_buffer():
    from pypanadapter_amd import ZoomFFT

    rows = _rows()
    plans = {name: ZoomFFT(N_FFT, ZOOM, FS, n_win=W) for name in ("all", "persistence", "detect", "viewport", "history")}
    try:
        _enable(plans["all"], ("persistence", "detect", "viewport", "history"))
        for name in ("persistence", "detect", "viewport", "history"):
            _enable(plans[name], (name,))
        owner = {"floors": "detect"}
        at = 0
        for b, n in enumerate(BATCHES):
            batch = rows[at:at + n]
            order = OPS[b % len(OPS):] + OPS[:b % len(OPS)]
            for k, op in enumerate(order):
                if k == READ_AFTER and at:  # the rows of the earlier batches, whatever this batch has pushed
                    _same_bits((plans["all"].history_rows(0, at),), (plans["history"].history_rows(0, at),),
                               f"batch {b}: history_rows(0, {at})")
                _same_bits(_call(plans["all"], op, batch), _call(plans[owner.get(op, op)], op, batch), f"batch {b}: {op}")
            at += n

        everything = ("persistence", "detect", "viewport", "history")
        got = _state(plans["all"], everything)
        for name in everything:
            for what, ref in _state(plans[name], (name,)).items():
                _same_bits(got[what], ref, what)
        assert got["persistence"][1] == at and got["detect_occupancy"][1] == at
        assert got["detect_occupancy"][0].any(), "the detector found nothing: the comparison is empty"

        # the viewport off: the shared staging is released under the other three; the next host
        # pushes allocate it again
        plans["all"].set_viewport(0, 0)
        tail = rows[at:at + TAIL]
        rest = ("persistence", "history")
        for op in rest:
            _same_bits(_call(plans["all"], op, tail), _call(plans[op], op, tail), f"tail: {op}")
        got = _state(plans["all"], rest)
        for name in rest:
            for what, ref in _state(plans[name], (name,)).items():
                _same_bits(got[what], ref, f"tail: {what}")
        assert plans["all"].history_state() == (at + TAIL, at + TAIL - 64)
    finally:
        for p in plans.values():
            p.close()
