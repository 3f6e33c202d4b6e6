"""GPU checks of the resampler bank (zfft_plan_resamp; csrc/resamp_kernels.hip) against the header's
arithmetic itself: resamp_ref's float32 model (tests/f32_exact.py) rounds where rules 2 and 4 of
include/zfft.h say the kernel rounds, so every comparison of outputs here is
`np.array_equal(got, want, equal_nan=True)` on float32 or int16 -- +0 equal to -0, because the
header does not fix the sign of a zero sum, and no tolerance.  No device library function stands
between input and output.

The chooser takes the form from the lane count alone (K >= 8: streams, K < 8: time), so one plan
cannot run one stream through both forms and hand the carry over; instead each form is held to the
model, and test_lane_subsets_in_place runs the same lanes of one array through the time form (3
lanes), the narrow streams form (8 lanes) and the wave-wide one (64 lanes) against the same model
columns."""
import functools

import numpy as np
import pytest

import resamp_ref as rr
import stall
from test_resamp_host import resamp_form

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu(zfft_lib):
    from pypanadapter_amd import device_count
    assert device_count() >= 1, "GPU tests need a HIP device"


def equal(got, want, what):
    assert rr.same(got, want), f"{what}: {rr.first_difference(got, want)}"


def _plan(K, L, M, T, h, fmt="f32", scale=32767.0):
    from pypanadapter_amd import ZoomFFT
    plan = ZoomFFT(32, 1, 1.0)
    plan.set_resamp(K, L, M, taps=h, taps_per_phase=T, format=fmt, scale=scale)
    assert plan.resamp_shape() == (K, L, M, T, plan.RESAMP_FORMATS[fmt])
    return plan


def _form(plan, n0=0, n=1, stride=None):
    K, L, M, T, fmt = plan.resamp_shape()
    return resamp_form(plan.lib, K, L, M, T, stride, fmt, n0, n)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda")


def _push_ptr(plan, ptr, n, stride):
    """One device push of n steps at `ptr`; (outputs, K) in the plan's format.  Nothing beyond
    outputs x K is written."""
    import torch
    K, fmt = plan.resamp_shape()[0], plan.resamp_shape()[4]
    outs, guard = plan.resamp_steps(n), 64
    d_r = stall.sentinel((outs * K + guard,), dtype=torch.int16 if fmt == rr.S16 else torch.float32)
    plan.resamp_push_device(ptr, n, stride, d_r.data_ptr())
    torch.cuda.synchronize()
    r = d_r.cpu().numpy()
    assert (r[outs * K:] == stall.SENTINEL).all()
    return r[:outs * K].reshape(outs, K).copy()


def _push(plan, x, stride=None):
    """One device push of the (steps, K) array, rows `stride` floats apart with NaN in the gaps."""
    n, K = x.shape
    stride = K if stride is None else stride
    buf = np.full((max(n, 1), stride), np.nan, np.float32)
    buf[:n, :K] = x
    d_x = _dev(buf)
    return _push_ptr(plan, d_x.data_ptr(), n, stride)


def push_cut(plan, x, cut=None, stride=None):
    """x pushed in pieces of `cut` steps (None: one push); the outputs back to back."""
    parts, at = [], 0
    for c in ([len(x)] if cut is None else cut):
        parts.append(_push(plan, x[at:at + c], stride))
        at += c
    assert at == len(x)
    return np.concatenate(parts)


@functools.lru_cache(maxsize=None)
def _case(i):
    """Case i's taps, input and model outputs (computed once; read-only)."""
    K, L, M, T, _ = rr.CASES[i]
    h = np.float32([1.0]) if L * T == 1 else rr.solid_taps(L, T)
    f = resamp_form(_lib(), K, L, M, T)
    n = rr.case_len(f["span"])
    x = rr.noise(n, K, 7 + i)
    want = rr.model_push(x, 0, h, L, M)
    for a in (h, x, want):
        a.setflags(write=False)
    return h, x, want


def _lib():
    from pypanadapter_amd import _lib as lib
    return lib.load()


# ---------------------------------------------------------------- 1. every case
@pytest.mark.parametrize("i", range(len(rr.CASES)), ids=rr.IDS)
def test_each_case_is_the_float32_rule(i):
    K, L, M, T, kind = rr.CASES[i]
    h, x, want = _case(i)
    with _plan(K, L, M, T, h) as plan:
        f = _form(plan, 0, len(x))
        assert f["kind"] == kind and f["nspans"] == 3 and len(x) % f["span"]     # two spans and a ragged part
        assert f["lane_tiles"] == -(-K // f["lanes"]) and (K != 70 or (f["lanes"] == 64 and f["lane_tiles"] == 2))
        assert plan.resamp_info() == {"group_delay": rr.group_delay(L, T), "rate_ratio": L / M}
        r = _push(plan, x)
        assert plan.resamp_state() == len(x)
    equal(r, want, rr.IDS[i])
    if L * T == 1:
        assert r.tobytes() == x.tobytes()                # 1 / 1 with h = [1]: the input itself, bytewise


def test_the_form_is_the_lane_count_alone():
    lib = _lib()
    for K in (1, 7, 8, 64, 2048):
        for stride in (K, K + 1, 4096, 2 ** 31):
            assert resamp_form(lib, K, 3, 4, 8, stride)["kind"] == (rr.STREAMS if K >= 8 else rr.TIME)


# ---------------------------------------------------------------- 2. cuts and counts, one case per form
@pytest.mark.parametrize("K,L,M,T,kind", [(64, 147, 250, 32, rr.STREAMS), (2, 147, 160, 16, rr.TIME)], ids=["streams", "time"])
def test_cuts_and_late_counts_are_the_float32_rule(K, L, M, T, kind):
    h = rr.solid_taps(L, T)
    starts = (0, 2 ** 32 - 100, 2 ** 62 - 10 ** 6)
    with _plan(K, L, M, T, h) as plan:
        f = _form(plan)
        span = f["span"]
        assert f["kind"] == kind
        cut = [1, M - 1, T - 1, T, span - 1, span + 1, 1]
        n = sum(cut) + span + 5
        cut.append(n - sum(cut))
        x = rr.noise(n, K, 38)
        got = {}
        for start in starts:
            plan.resamp_reset(start)
            got[start, "whole"] = push_cut(plan, x)
            assert plan.resamp_state() == start + n
            plan.resamp_reset(start)
            got[start, "cut"] = push_cut(plan, x, cut)
            assert plan.resamp_state() == start + n
    for start in starts:
        want = rr.model_push(x, start, h, L, M)
        equal(got[start, "whole"], want, f"whole at {start}")
        equal(got[start, "cut"], want, f"cut at {start}")


# ---------------------------------------------------------------- 3. S16
@pytest.mark.parametrize("K,L,M,T", [(8, 16, 25, 32), (1, 3, 4, 8)], ids=["streams", "time"])
def test_s16_is_the_models_codes(K, L, M, T):
    h = rr.solid_taps(L, T)
    x = rr.noise(1500, K, 51)
    y = rr.model_push(x, 0, h, L, M)
    scale = float(np.float32(20000.0 / y.std()))          # the rails at 1.6 sigma of the input's own model
    want = rr.quantise(y, scale)
    assert (want == 32767).any() and (want == -32768).any() and (np.abs(want) < 32767).mean() > 0.5   # both rails, mostly inside
    with _plan(K, L, M, T, h, "s16", scale) as plan:
        q = push_cut(plan, x, [700, 800])
    assert q.dtype == np.int16
    equal(q, want, "S16 codes")
    with _plan(K, L, M, T, h) as plan:                    # the float32 plan, quantised by the host rule
        equal(rr.quantise(_push(plan, x), scale), q, "float32 then the host rule")


@pytest.mark.parametrize("K", [8, 1], ids=["streams", "time"])
def test_s16_ties_nan_and_infinities(K):
    k = np.arange(-40, 40, dtype=np.float32)
    col = np.concatenate([k + np.float32(0.5), [32766.5, 32767.5, -32767.5, -32768.5, 40000.0, -40000.0, 3e38, -3e38,
                                                np.nan, np.inf, -np.inf, 0.0, -0.0, 0.49999997, -0.49999997]]).astype(np.float32)
    x = np.stack([np.roll(col, s) for s in range(K)], axis=1)
    with _plan(K, 1, 1, 1, np.float32([1.0]), "s16", 1.0) as plan:     # y = fma(1, x, +0) = x, scale 1
        q = _push(plan, x)
    want = rr.quantise(x, 1.0)
    assert want[:4, 0].tolist() == [-40, -38, -38, -36]   # -39.5 -> -40, -38.5 -> -38, -37.5 -> -38: ties to even
    at = {float(v) if np.isfinite(v) else str(v): int(c) for v, c in zip(col, want[:, 0])}
    assert at["nan"] == 0 and at["inf"] == 32767 and at["-inf"] == -32768 and at[32767.5] == 32767 and at[-32768.5] == -32768
    equal(q, want, "ties, NaN and the infinities")


# ---------------------------------------------------------------- 4. containment
@pytest.mark.parametrize("K,L,M,T", [(16, 16, 25, 8), (3, 3, 4, 8)], ids=["streams", "time"])
def test_a_nan_or_an_inf_stays_in_its_lane_and_its_window(K, L, M, T):
    h = rr.solid_taps(L, T).copy()
    h[3 * L:4 * L] = 0.0                                  # tap 3 of every phase is zero: 0 x NaN must still be formed
    with _plan(K, L, M, T, h) as plan:
        span = _form(plan)["span"]
        n = span + 300
        p = span - 1                                      # the last step of a span: the window reaches into the next
        base_x = rr.noise(n, K, 19)
        base = _push(plan, base_x)
        i_m = np.array(rr.positions(rr.out_indices(0, n, L, M), L, M)[0])
        inside = (i_m >= p) & (i_m <= p + T - 1)
        assert inside.sum() >= T * L // M
        for s in (0, K - 1):
            for bad in (np.nan, np.inf):
                x = base_x.copy()
                x[p, s] = bad
                plan.resamp_reset(0)
                r = push_cut(plan, x, [p + 1, n - p - 1])  # the bad sample goes through the carry
                others = np.arange(K) != s
                assert r[:, others].tobytes() == base[:, others].tobytes(), f"the other lanes, {bad} in lane {s}"
                assert r[~inside, s].tobytes() == base[~inside, s].tobytes(), f"lane {s} outside the window of its {bad}"
                assert not np.isfinite(r[inside, s]).any()  # the zero coefficient included
                with np.errstate(all="ignore"):
                    equal(r[:, s:s + 1], rr.model_push(x[:, s:s + 1], 0, h, L, M), f"lane {s} with its {bad}")


# ---------------------------------------------------------------- 5. strides
@pytest.mark.parametrize("i", [1, 6], ids=["time", "streams"])
def test_a_padded_stride_with_nan_in_the_gaps(i):
    K, L, M, T, _ = rr.CASES[i]
    h, x, want = _case(i)
    with _plan(K, L, M, T, h) as plan:
        equal(push_cut(plan, x, [len(x) // 2, len(x) - len(x) // 2], stride=K + 13), want, f"{rr.IDS[i]} at stride K + 13")


def test_lane_subsets_in_place():
    """8 and 3 neighbouring lanes of a 64-wide array by pointer offset and the array's stride, against
    the columns of the model of all 64: the wave-wide streams form, the narrow one and the time form
    give the same bits."""
    L, M, T = 16, 25, 32
    h = rr.solid_taps(L, T)
    x = rr.noise(700, 64, 77)
    d_x = _dev(x)
    want = rr.model_push(x, 0, h, L, M)
    kinds = {}
    for K, off in ((64, 0), (8, 24), (3, 41)):
        with _plan(K, L, M, T, h) as plan:
            f = _form(plan, 0, 700, 64)
            kinds[K] = (f["kind"], f["lanes"])
            r = np.concatenate([_push_ptr(plan, d_x.data_ptr() + 4 * off, 300, 64),
                                _push_ptr(plan, d_x.data_ptr() + 4 * (300 * 64 + off), 400, 64)])
        equal(r, want[:, off:off + K], f"{K} lanes at {off}")
    assert kinds == {64: (rr.STREAMS, 64), 8: (rr.STREAMS, 8), 3: (rr.TIME, 3)}


def test_a_stride_that_puts_the_last_sample_past_4_gib():
    import torch
    K, L, M, T, n, stride = 8, 3, 4, 8, 70, 1 << 24
    assert (n - 1) * stride * 4 > 2 ** 32
    h = rr.solid_taps(L, T)
    x = rr.noise(n, K, 88)
    try:
        d_x = torch.empty(((n - 1) * stride + K,), dtype=torch.float32, device="cuda")
    except torch.cuda.OutOfMemoryError:
        pytest.skip("no 4.4 GiB of device memory for the input")
    d_x.as_strided((n, K), (stride, 1)).copy_(_dev(x))    # laid out on the device
    with _plan(K, L, M, T, h) as plan:
        r = _push_ptr(plan, d_x.data_ptr(), n, stride)
    equal(r, rr.model_push(x, 0, h, L, M), "stride 2^24")


# ---------------------------------------------------------------- 6. short pushes
@pytest.mark.parametrize("K", [16, 5], ids=["streams", "time"])
def test_short_pushes_and_pushes_that_emit_nothing(K):
    L, M, T = 1, 7, 24
    h = rr.solid_taps(L, T)
    cut = [1, 2, 3, 1, 5, 0, 22, 1, 1, 1, 0, 6, 23, 40, 2, 1, 100]   # most below T - 1 = 23, several emit nothing
    x = rr.noise(sum(cut), K, 61)
    with _plan(K, L, M, T, h) as plan:
        counts = []
        at = 0
        parts = []
        for c in cut:
            counts.append(plan.resamp_steps(c))
            parts.append(_push(plan, x[at:at + c]))
            at += c
            assert plan.resamp_state() == at
        assert counts == [rr.steps(sum(cut[:j]), c, L, M) for j, c in enumerate(cut)] and counts.count(0) >= 8
        plan.resamp_push_device(0, 0, K, 0)              # steps = 0: ZFFT_OK, nothing happens
        assert plan.resamp_state() == at
    equal(np.concatenate(parts), rr.model_push(x, 0, h, L, M), "short pushes")


# ---------------------------------------------------------------- 7. more tiles than the grid
def test_more_tiles_than_workgroups():
    """The smallest shape whose tiles pass the grid's 65536: 2048 lanes are 32 lane tiles of 64, and
    the shortest span of 64-lane tiles is 80 steps (T = 81: a shorter one would halve the lanes), so
    2049 spans.  M = 16 keeps the output small.  Whole lanes against the model at the first and
    last spans and where the second round of tiles begins (tile 65536 = span 2048)."""
    import torch
    K, L, M, T = 2048, 1, 16, 81
    h = rr.solid_taps(L, T)
    with _plan(K, L, M, T, h) as plan:
        f = _form(plan)
        span = f["span"]
        n = 2048 * span + span // 2
        f = _form(plan, 0, n)
        assert (f["lanes"], span, f["lane_tiles"]) == (64, 80, 32) and f["ntiles"] > f["grid"] == 1 << 16
        assert _form(plan, 0, n - span)["ntiles"] <= 1 << 16         # one span fewer fits the grid
        try:
            g = torch.Generator(device="cuda").manual_seed(5)
            d_x = torch.rand((n, K), generator=g, device="cuda", dtype=torch.float32).mul_(2.0).sub_(1.0)
        except torch.cuda.OutOfMemoryError:
            pytest.skip("no 1.4 GiB of device memory for the input")
        r = _push_ptr(plan, d_x.data_ptr(), n, K)
    ms = rr.out_indices(0, n, L, M)
    i_m = np.array(rr.positions(ms, L, M)[0])
    round2 = (1 << 16) // f["lane_tiles"]                 # the span of tile 65536
    assert round2 == 2048
    for lo, hi in ((0, 2 * span), ((round2 - 1) * span, n), (n - span - span // 2, n)):
        first = max(0, lo - (T - 1))
        x = d_x[first:hi].cpu().numpy()
        pick = np.nonzero((i_m >= lo) & (i_m < hi))[0]
        want = rr.model_resamp(x, first, h, L, M, [ms[j] for j in pick])
        assert pick.size >= span // M
        equal(r[pick], want, f"steps [{lo}, {hi})")


# ---------------------------------------------------------------- 8. ordering
@pytest.mark.parametrize("reset", [False, True], ids=["push", "reset-between"])
def test_a_device_push_behind_a_stalled_stream(reset):
    """demod_push_device on A and, right after it, a resampler push on B that reads its output and
    another on C, enqueued while a bounded spin kernel holds A (tests/stall.py), then a synchronous
    host push behind them: nothing runs ahead of the plan's earlier work and the results equal the
    stepped run's bytewise -- also with a resamp_reset enqueued between the two device pushes."""
    import torch
    import demod_ref as dr
    from pypanadapter_amd import ZoomFFT
    streams = stall.streams()
    K, Ta, Da, L, M, T = 16, 33, 4, 3, 4, 8
    x = dr.noise_and_tones(3000, K, 37)
    g, h = dr.audio_taps(Ta, Da), rr.solid_taps(L, T)
    tail = rr.noise(200, K, 5)
    na = dr.steps(0, 3000, Da)
    n1 = 401

    def bufs():
        return {"x": torch.from_numpy(x.view(np.float32).reshape(-1, 2).copy()).to("cuda"), "a": stall.sentinel((na * K,)),
                "r": stall.sentinel((2 * rr.steps(0, na, L, M) * K,))}

    def seq(plan, run, b):
        run.call("demod_push", plan.demod_push_device, b["x"].data_ptr(), 3000, K, 1, b["a"].data_ptr(), on=streams[0])
        run.call("resamp_push0", plan.resamp_push_device, b["a"].data_ptr(), n1, K, b["r"].data_ptr(), on=streams[1])
        if reset:
            run.host(plan.resamp_reset, n1)
        o1 = rr.steps(0, n1, L, M)
        run.call("resamp_push1", plan.resamp_push_device, b["a"].data_ptr() + 4 * n1 * K, na - n1, K,
                 b["r"].data_ptr() + 4 * o1 * K, on=streams[2])

    def make():
        plan = ZoomFFT(32, 1, 1.0)
        plan.set_demod(K, taps=g, decim=Da)
        plan.set_resamp(K, L, M, taps=h, taps_per_phase=T)
        seq(plan, stall.Run(plan, streams, held=False), bufs())   # the workspaces have their size
        plan.resamp_push(tail)
        torch.cuda.synchronize()
        plan.demod_reset(0)
        plan.resamp_reset(0)
        torch.cuda.synchronize()
        return plan, bufs()

    def sequence(plan, run, b):
        seq(plan, run, b)
        run.check_order()
        if run.held:
            assert stall.quiesce_count(plan) == run.q0            # no host wait in any enqueue, the reset's included
        after = run.waiting("resamp_push_host", plan.resamp_push, tail)
        return {"a": b["a"], "r": b["r"], "after": after, "steps": plan.resamp_state()}

    held, stepped, run = stall.enqueue_twice(f"resamp[{'reset' if reset else 'push'}]", make, sequence, streams)
    stall.same_bytes(held, stepped, "held")
    a = held["a"].reshape(na, K)
    assert not (a == stall.SENTINEL).any()
    outs = rr.steps(0, na, L, M)
    r = held["r"][:outs * K].reshape(outs, K)
    if reset:                                                     # the second push starts again, at count n1, from a zero past
        want = np.concatenate([rr.model_push(a[:n1], 0, h, L, M), rr.model_push(a[n1:], n1, h, L, M)])
        after = rr.model_resamp(np.concatenate([a[n1:], tail]), n1, h, L, M, rr.out_indices(na, len(tail), L, M))
    else:
        want = rr.model_push(a, 0, h, L, M)
        after = rr.model_resamp(np.concatenate([a, tail]), 0, h, L, M, rr.out_indices(na, len(tail), L, M))
    assert held["steps"] == na + len(tail)
    equal(r, want, "the two pushes behind the held stream")
    equal(held["after"], after, "the host push behind them")


# ---------------------------------------------------------------- 9. end to end
def _tone(a, f, skip):
    """The amplitude of the tone at f cycles per sample in a[skip:] (real: both lines), by a heavy window."""
    s = np.asarray(a[skip:])
    w = np.blackman(s.size) * np.kaiser(s.size, 20.0)
    w /= w.sum()
    return (1.0 if np.iscomplexobj(s) else 2.0) * abs(np.sum(w * s.astype(np.complex128) * np.exp(-2j * np.pi * f * np.arange(s.size))))


FLOOR = 1e-6   # the window's leakage of neighbouring lines (-150 dB) and the input's float32 rounding


def _tone_bound(h, L, f, amp, real):
    """What the prototype may move a tone of amplitude amp at f cycles per input sample by: its
    passband ripple at f / L, every image (k +- f) / L, 0 < k < L, of the tone's lines (a real tone
    has two) at the prototype's response there -- wherever the decimation then puts them -- and
    rule 7's gate."""
    k = np.arange(1, L)
    images = np.concatenate([(k + f) / L, (k - f) / L] if real else [(k + f) / L])
    rho = abs(rr.response(h, f / L)[0] / L - 1.0)
    leak = float(rr.response(h, images).sum()) / L if L > 1 else 0.0
    return amp * (rho + leak) + rr.gate(h, L, amp) + FLOOR, rho


def test_end_to_end_channeliser_demodulator_resampler():
    """An FM carrier in one channel of a (64, 8, 32) bank at 2.4 MHz: Channelizer ->
    Demodulator.for_channelizer(.., "fm", audio_decim=4) -> Resampler.for_demodulator(.., 48 kHz), the
    ratio 64 / 25.  The chain's output is resamp_ref's model of the demodulator's own output, bit for
    bit, and the audio tone sits at f_a 25 / 64 cycles per output sample with the amplitude it had
    before, within what the prototype's ripple at that frequency, its images and rule 7 allow."""
    from pypanadapter_amd import Channelizer, Demodulator, Resampler, resamp_design
    fs, Mc, D, Da, c, f_d, beta = 2.4e6, 64, 32, 4, 5, 0.01, 1.0
    n = 3200 * D
    t = np.arange(n, dtype=np.float64)
    x = (0.5 * np.exp(1j * (2 * np.pi * (c / Mc) * t + beta * np.sin(2 * np.pi * (f_d / D) * t)))).astype(np.complex64)
    bank = Channelizer(fs, Mc, ascending=False)
    try:
        audio = Demodulator.for_channelizer(bank, "fm", audio_decim=Da)
        pcm = Resampler.for_demodulator(audio, 48e3)
        assert (pcm.L, pcm.M, pcm.lanes) == (64, 25, Mc) and pcm.rate == 48e3 and audio.rate == 18750.0
        T = rr.default_taps_per_phase(64, 25)
        assert bank._plan.resamp_shape() == (Mc, 64, 25, T, 0) and pcm.group_delay == rr.group_delay(64, T)
        y = bank.push(x)
        a = audio.push(y)
        r = np.concatenate([pcm.push(a[:301]), pcm.push(a[301:])])
        assert pcm.steps_seen == len(a) and pcm.steps(25) == 64
        h = resamp_design(64, 25).astype(np.float32)
        equal(r, rr.model_push(a, 0, h, 64, 25), "the chain against the model of its own audio")
        f_a = f_d * Da                                   # cycles per audio sample
        skip = 64
        amp = _tone(a[:, c], f_a, skip)
        got = _tone(r[:, c], f_a * 25 / 64, skip * 64 // 25)
        bound, rho = _tone_bound(h, 64, f_a, amp, real=True)
        print(f"audio tone {amp:.7f} -> {got:.7f} at 48 kHz (ripple {rho:.2e}): |diff| {abs(got - amp):.2e} of {bound:.2e}")
        assert amp > 0.005 and abs(got - amp) <= bound < 0.01 * amp
        # ... and nowhere else: the image nearest in frequency is gone
        assert _tone(r[:, c], (1 - f_a) * 25 / 64, skip * 64 // 25) <= bound
        pcm.close()
        with pytest.raises(ValueError, match="resamp is off"):
            bank._plan.resamp_state()
        s16 = Resampler.for_demodulator(audio, 48e3, format="s16")
        audio.reset()
        q = s16.push(audio.push(y))
        equal(q, rr.quantise(rr.model_push(a, 0, h, 64, 25)), "int16 PCM at 48 kHz")
    finally:
        bank.close()


def test_end_to_end_tap_resampler_complex():
    """One tap at fs / 32 = 75 kHz to 48 kHz IQ, 16 / 25: complex in, complex out.  The output is the
    model of the tap's own output as two lanes, and a carrier 0.02 cycles per tap sample off the
    tap's centre sits at 0.02 x 25 / 16 with its amplitude."""
    from pypanadapter_amd import Resampler, Tap, resamp_design
    fs, D, off = 2.4e6, 32, 0.02
    n = 3000 * D
    x = (0.5 * np.exp(2j * np.pi * ((0.1 + off / D) * np.arange(n)))).astype(np.complex64)
    taps = Tap(fs, max_taps=2, max_len=8 * D + 1)
    try:
        taps.open(1, 0.1 * fs, decim=D)
        iq = Resampler.for_tap(taps, 48e3)
        assert (iq.L, iq.M, iq.lanes, iq.rate) == (16, 25, 2, 48e3)
        y = taps.push(x)[1]
        r = np.concatenate([iq.push(y[:1000]), iq.push(y[1000:])])
        assert r.dtype == np.complex64 and r.shape == (rr.steps(0, len(y), 16, 25), 1)
        h = resamp_design(16, 25).astype(np.float32)
        lanes = np.ascontiguousarray(y).view(np.float32).reshape(-1, 2)
        equal(np.ascontiguousarray(r).view(np.float32).reshape(-1, 2), rr.model_push(lanes, 0, h, 16, 25), "tap -> resampler")
        skip = 64
        amp = _tone(y, off, skip)
        got = _tone(r[:, 0], off * 25 / 16, skip * 16 // 25)
        bound, rho = _tone_bound(h, 16, off, amp, real=False)
        print(f"carrier {amp:.7f} -> {got:.7f} at 48 kHz (ripple {rho:.2e}): |diff| {abs(got - amp):.2e} of {bound:.2e}")
        assert amp > 0.4 and abs(got - amp) <= bound < 0.01 * amp
    finally:
        taps.close()


# ---------------------------------------------------------------- 10. off means off; calls and errors
def test_off_means_off():
    from pypanadapter_amd import ZoomFFT, synth
    x = np.stack([synth.make_iq(65536, 2.4e6, 3 + f, n_fft=1024, zoom=8, n_win=128) for f in range(16)])
    y = rr.noise(500, 4, 3)
    with ZoomFFT(1024, 8, 2.4e6, n_win=128) as plan:
        plan.set_timing(True)
        rows = plan.rows(x)
        names = plan.launch_names()
        assert names and not [n for n in names if "resamp" in n]

        def off():
            assert plan.lib.zfft_resamp_shape is not None
            for call in (plan.resamp_state, plan.resamp_shape, lambda: plan.resamp_steps(5), lambda: plan.resamp_push(y),
                         plan.resamp_info, plan.resamp_reset, lambda: plan.resamp_push_device(8, 1, 4, 8)):
                with pytest.raises(ValueError, match="resamp is off"):
                    call()
        off()
        plan.set_resamp(4, 3, 4)                          # on: a process call is still the plan's alone
        assert plan.resamp_shape() == (4, 3, 4, 32, 0)
        assert np.array_equal(plan.rows(x), rows) and plan.launch_names() == names
        r = plan.resamp_push(y)
        assert plan.launch_names() == ["resamp_push"] and len(plan.timings()) == 1 and r.shape == (375, 4)
        plan.set_resamp(0)                                # off again, everything freed
        off()
        assert np.array_equal(plan.rows(x), rows) and plan.launch_names() == names
        plan.set_resamp(0)


def test_calls_and_errors():
    import ctypes
    from pypanadapter_amd import ZoomFFT, _lib
    with ZoomFFT(32, 1, 1.0) as plan:
        h = np.ones(8192, np.float32)
        p = h.ctypes.data_as(ctypes.c_void_p)
        for K, L, M, T, fmt in [(-1, 3, 4, 8, 0), (2049, 3, 4, 8, 0), (4, 0, 4, 8, 0), (4, 513, 4, 8, 0), (4, 3, 0, 8, 0),
                                (4, 3, 4097, 8, 0), (4, 2, 4, 8, 0), (4, 6, 9, 8, 0), (4, 3, 4, 0, 0), (4, 3, 4, 129, 0),
                                (4, 512, 1, 17, 0), (4, 3, 4, 8, 2), (4, 3, 4, 8, -1)]:
            assert plan.lib.zfft_plan_resamp(plan._plan, K, L, M, T, p, fmt, 1.0) == _lib.ZFFT_EINVAL, (K, L, M, T, fmt)
        assert b"resamp" in plan.lib.zfft_last_error()
        assert plan.lib.zfft_plan_resamp(plan._plan, 4, 3, 4, 8, None, 0, 1.0) == _lib.ZFFT_EINVAL    # without taps: 0 or the default's
        assert plan.lib.zfft_plan_resamp(plan._plan, 4, 1, 16, 0, None, 0, 1.0) == _lib.ZFFT_EINVAL   # a default that does not fit
        with pytest.raises(ValueError, match="resamp is off"):
            plan.resamp_state()                           # a refused call enables nothing
        plan.set_resamp(4, 6, 8)                          # the wrapper reduces the fraction
        assert plan.resamp_shape() == (4, 3, 4, 32, 0) and plan.resamp_state() == 0
        plan.set_resamp(3, 2, 1, taps=h[:10], format="s16", scale=100.0)
        assert plan.resamp_shape() == (3, 2, 1, 5, 1)
        d = _dev(np.zeros((16, 3)))
        for bad in [(d.data_ptr(), 4, 2, d.data_ptr()), (d.data_ptr(), 4, 2 ** 31 + 1, d.data_ptr()), (0, 4, 3, d.data_ptr()),
                    (d.data_ptr() + 2, 4, 3, d.data_ptr()), (d.data_ptr(), 4, 3, d.data_ptr() + 1), (d.data_ptr(), -1, 3, d.data_ptr()),
                    (d.data_ptr(), 2 ** 31, 3, d.data_ptr()), (d.data_ptr(), 4, 3, 0)]:
            with pytest.raises(ValueError, match="resamp"):
                plan.resamp_push_device(*bad)
        with pytest.raises(ValueError, match="n0 in"):
            plan.resamp_reset(2 ** 62 + 1)
        plan.resamp_reset(2 ** 62 - 3)
        with pytest.raises(ValueError, match="count would pass"):
            plan.resamp_push(np.zeros((4, 3), np.float32))
        assert plan.resamp_push(np.zeros((3, 3), np.float32)).shape == (6, 3) and plan.resamp_state() == 2 ** 62
        # complex in, complex out: two lanes a stream
        plan.set_resamp(2, 1, 1, taps=np.float32([1.0]))
        z = (rr.noise(50, 1, 1)[:, 0] + 1j * rr.noise(50, 1, 2)[:, 0]).astype(np.complex64)
        out = plan.resamp_push(z)
        assert out.dtype == np.complex64 and out.shape == (50, 1) and out[:, 0].tobytes() == z.tobytes()
