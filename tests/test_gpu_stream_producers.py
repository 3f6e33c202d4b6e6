"""GPU check that the three producers on a sample stream -- the channel taps, the channeliser and
the demodulator bank -- keep counts, carries and staging of their own behind the host path they
share (csrc/zfft_stream.cpp); the sample side's counterpart of test_gpu_shared_staging.py.  One
plan has all three on, three more plans one each.  A seeded stream of 3000 samples (the bank: the
same values as 1000 steps of 3 streams) is pushed from the host in cuts of 1, 2, 15, 16, 700, 1
and the rest -- every staging grows, then is used far below its size, and the 700 crosses a span
boundary of the taps -- to every producer, in an order that rotates from cut to cut.  Everything
the shared plan returns must equal, bit for bit, what the single-producer plans return; their own
suites tie those to the references.  Then a reset of one producer leaves the counts of the other
two alone, and switching the taps off leaves the other two as they were."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N = 3000
CUTS = (1, 2, 15, 16, 700, 1)  # then the rest: 2265 samples, 265 steps of the bank
OPS = ("tap", "chan", "demod")
TAIL = 48  # samples (16 steps of the bank) pushed after the reset and again after the taps went off


def _stream():
    rng = np.random.default_rng(20240917)
    return (rng.standard_normal(N) + 1j * rng.standard_normal(N)).astype(np.complex64)


def _enable(plan, which):
    if "tap" in which:
        plan.set_taps(2, 9)
        plan.tap_open(0, 0.1, 3, taps=np.hanning(11)[1:-1])  # D = 3, T = 9
        plan.tap_open(1, -0.25, 1, taps=[1.0])               # D = 1, T = 1
    if "chan" in which:
        plan.set_channels(8, 2, oversample=2)
    if "demod" in which:
        plan.set_demod(3, taps=[0.1, 0.2, 0.4, 0.2, 0.1], decim=2)
        plan.demod_mode("fm", first=1, count=1)
        plan.demod_mode("ssb", bfo_hz=0.05, first=2)


def _call(plan, op, x, lo, hi):
    """One host push of the cut [lo, hi) of the stream (the bank: of its steps); what it returns,
    as a tuple of arrays."""
    if op == "tap":
        return tuple(plan.tap_push(x[lo:hi]))
    if op == "chan":
        return (plan.chan_push(x[lo:hi]),)
    return (plan.demod_push(x.reshape(-1, 3)[lo:hi]),)


def _same_bits(got, ref, what):
    assert len(got) == len(ref), what
    for k, (a, b) in enumerate(zip(got, ref)):
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}[{k}]"
        assert a.tobytes() == b.tobytes(), f"{what}[{k}] differs"


def test_three_producers_behind_one_host_path():
    from pypanadapter_amd import ZoomFFT

    x = _stream()
    plans = {name: ZoomFFT(32, 1, 1.0) for name in ("all",) + OPS}
    try:
        _enable(plans["all"], OPS)
        for name in OPS:
            _enable(plans[name], (name,))
        at = {op: 0 for op in OPS}
        end = {"tap": N, "chan": N, "demod": N // 3}
        outputs = {op: 0 for op in OPS}
        for b, cut in enumerate(CUTS + (N,)):
            order = OPS[b % 3:] + OPS[:b % 3]
            for op in order:
                lo, hi = at[op], min(at[op] + cut, end[op])
                got = _call(plans["all"], op, x, lo, hi)
                _same_bits(got, _call(plans[op], op, x, lo, hi), f"cut {b}: {op}")
                outputs[op] += sum(a.size for a in got)
                at[op] = hi
        assert at == end
        assert outputs == {"tap": N // 3 + N, "chan": N // 4 * 8, "demod": N // 3 // 2 * 3}, "an empty comparison"
        states = lambda p: (p.tap_state(), p.chan_state(), p.demod_state())
        assert states(plans["all"]) == (N, N, N // 3)

        # a reset of one producer: the other two keep their counts (and, below, their carries)
        for name in ("all", "chan"):
            plans[name].chan_reset(5)
        assert states(plans["all"]) == (N, 5, N // 3)
        for op in OPS:
            hi = TAIL // 3 if op == "demod" else TAIL
            _same_bits(_call(plans["all"], op, x, 0, hi), _call(plans[op], op, x, 0, hi), f"after chan_reset: {op}")

        # the taps off: the channeliser and the bank go on as if nothing had happened
        plans["all"].set_taps(0, 0)
        for op in ("demod", "chan"):
            hi = TAIL // 3 if op == "demod" else TAIL
            _same_bits(_call(plans["all"], op, x, 0, hi), _call(plans[op], op, x, 0, hi), f"taps off: {op}")
        assert (plans["all"].chan_state(), plans["all"].demod_state()) == (5 + 2 * TAIL, N // 3 + 2 * (TAIL // 3))
        with pytest.raises(ValueError, match="taps are off"):
            plans["all"].tap_push(x[:4])
    finally:
        for p in plans.values():
            p.close()
