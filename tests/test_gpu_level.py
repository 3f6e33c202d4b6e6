"""GPU checks of the level bank (zfft_plan_level; csrc/level_kernels.hip) against the header's
arithmetic itself: level_ref's float32 model rounds where rules 3 to 6 of include/zfft.h say the
kernels round, so every comparison of outputs here is `np.array_equal(got, want, equal_nan=True)`
on float32 -- +0 equal to -0, and no tolerance.

The chooser takes the form from the lane count alone (K >= 8: streams, K < 8: time), so each form is
held to the model, and test_lane_subsets_in_place runs the same lanes of one array through the
time form (3 lanes), the narrow streams form (8 lanes) and the wave-wide one (64 lanes) against the
same model columns."""
import functools

import numpy as np
import pytest

import level_ref as lr
import stall
from test_level_host import level_form

pytestmark = pytest.mark.gpu

# (K, B, H, form): the smallest shapes at which each mechanism can go wrong
SHAPES = [(1, 8, 0, lr.TIME), (2, 8, 1, lr.TIME), (3, 16, 5, lr.TIME), (7, 64, 2, lr.TIME), (8, 8, 0, lr.STREAMS),
          (64, 64, 5, lr.STREAMS), (100, 16, 40, lr.STREAMS), (2048, 8, 3, lr.STREAMS)]
IDS = [f"K{K}-B{B}-H{H}" for K, B, H, _ in SHAPES]
STARTS = (0, 5, 2 ** 32 - 100, 2 ** 62 - 10 ** 6, 2 ** 62 - 10 ** 6 + 7)
PAR = dict(target=0.5, gmax=1e4, floor=1e-6, squelch=3e-4)       # the squelch closes the quietest stretches


@pytest.fixture(scope="module", autouse=True)
def _gpu(zfft_lib):
    from pypanadapter_amd import device_count
    assert device_count() >= 1, "GPU tests need a HIP device"


def equal(got, want, what):
    assert lr.same(got, want), f"{what}: {lr.first_difference(got, want)}"


def _plan(K, B, H, **par):
    from pypanadapter_amd import ZoomFFT
    plan = ZoomFFT(32, 1, 1.0)
    p = {**PAR, **par}
    plan.set_level(K, B, H, **p)
    assert plan.level_shape() == (K, B, H) + tuple(float(np.float32(p[k])) for k in ("target", "gmax", "floor", "squelch"))
    return plan


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda")


def _push_ptr(plan, ptr, n, stride, key_ptr=0, key_stride=0):
    """One device push of n steps at `ptr`; (emitted, K) float32.  Nothing beyond emitted x K is written."""
    import torch
    K = plan.level_shape()[0]
    outs, guard = plan.level_steps(n), 64
    d_r = stall.sentinel((outs * K + guard,))
    plan.level_push_device(ptr, n, stride, d_r.data_ptr(), key_ptr, key_stride)
    torch.cuda.synchronize()
    r = d_r.cpu().numpy()
    assert (r[outs * K:] == stall.SENTINEL).all()
    return r[:outs * K].reshape(outs, K).copy()


def _padded(x, stride):
    n, K = x.shape
    buf = np.full((max(n, 1), stride), np.nan, np.float32)
    buf[:n, :K] = x
    return _dev(buf)


def _push(plan, x, key=None, stride=None, key_stride=None):
    """One device push of the (steps, K) array, rows `stride` floats apart with NaN in the gaps."""
    n, K = x.shape
    stride = K if stride is None else stride
    d_x = _padded(x, stride)
    if key is None:
        return _push_ptr(plan, d_x.data_ptr(), n, stride)
    key_stride = K if key_stride is None else key_stride
    d_k = _padded(key, key_stride)
    return _push_ptr(plan, d_x.data_ptr(), n, stride, d_k.data_ptr(), key_stride)


def push_cut(plan, x, cut=None, key=None, **kw):
    """x pushed in pieces of `cut` steps (None: one push); the outputs back to back."""
    parts, at = [], 0
    for c in ([len(x)] if cut is None else cut):
        parts.append(_push(plan, x[at:at + c], None if key is None else key[at:at + c], **kw))
        at += c
    assert at == len(x)
    return np.concatenate(parts)


@functools.lru_cache(maxsize=None)
def _case(i):
    """Shape i's input (some 30 blocks and a ragged part) and its model outputs at start 0 (computed once; read-only)."""
    K, B, H, _ = SHAPES[i]
    n = 30 * B + B // 2 + 1 if K <= 100 else 24 * B + 3
    x = lr.noise(n, K, 11 + i)
    want = lr.model_push(x, 0, B, H, **PAR)
    for a in (x, want):
        a.setflags(write=False)
    return x, want


# ---------------------------------------------------------------- 1. every shape
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_each_shape_is_the_float32_rule(i):
    K, B, H, kind = SHAPES[i]
    x, want = _case(i)
    assert (want == 0).any() and (np.abs(want) > 0.4).any()        # the squelch closes somewhere, the target is reached
    with _plan(K, B, H) as plan:
        f = level_form(plan.lib, K, B, H, 0, 0, len(x))
        assert f["kind"] == kind and f["outs"] == len(want) == lr.steps(0, 0, len(x), B)
        assert plan.level_info() == {"latency_min": float(B), "latency_max": 2.0 * B - 1, "rate_ratio": 1.0}
        r = _push(plan, x)
        assert plan.level_state() == len(x)
    equal(r, want, IDS[i])


# ---------------------------------------------------------------- 2. cuts and counts, every shape
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_cuts_and_late_counts_are_the_float32_rule(i):
    K, B, H, _ = SHAPES[i]
    x, _ = _case(i)
    cut = [1, B - 1, B, B + 1, 2 * B - 1, 2 * B, 3]
    cut.append(len(x) - sum(cut))
    assert cut[-1] > 2 * B
    got = {}
    starts = STARTS if K <= 100 else STARTS[2:4]          # (2048 lanes: two late starts, one of them unaligned)
    with _plan(K, B, H) as plan:
        for start in starts:
            plan.level_reset(start)
            got[start, "whole"] = push_cut(plan, x)
            assert plan.level_state() == start + len(x)
            plan.level_reset(start)
            counts = []
            at, parts = 0, []
            for c in cut:
                counts.append(plan.level_steps(c))
                parts.append(_push(plan, x[at:at + c]))
                at += c
            assert counts == [lr.steps(start + sum(cut[:j]), start, c, B) for j, c in enumerate(cut)]
            got[start, "cut"] = np.concatenate(parts)
    assert any(s % B for s in starts)                     # unaligned starts among them
    for start in starts:
        want = lr.model_push(x, start, B, H, **PAR)
        equal(got[start, "whole"], want, f"whole at {start}")
        equal(got[start, "cut"], want, f"cut at {start}")


# ---------------------------------------------------------------- 3. short and empty pushes
@pytest.mark.parametrize("K,B,H", [(16, 8, 3), (5, 8, 3)], ids=["streams", "time"])
def test_short_pushes_and_pushes_that_emit_nothing(K, B, H):
    cut = [1] * (3 * B + 2) + [B - 1, 1, 0, 2, B - 3, 1, 2 * B - 1, 1, 3 * B, 1, 1, 40]
    x = lr.noise(sum(cut), K, 61)
    for start in (0, 3):
        with _plan(K, B, H) as plan:
            plan.level_reset(start)
            counts, parts, at = [], [], 0
            for c in cut:
                counts.append(plan.level_steps(c))
                parts.append(_push(plan, x[at:at + c]))
                at += c
                assert plan.level_state() == start + at
            assert counts == [lr.steps(start + sum(cut[:j]), start, c, B) for j, c in enumerate(cut)]
            assert counts.count(0) >= 3 * B - 2 and (start or set(counts[:3 * B + 2]) == {0, B})
            plan.level_push_device(0, 0, K, 0)           # steps = 0: ZFFT_OK, nothing happens
            assert plan.level_state() == start + at
        equal(np.concatenate(parts), lr.model_push(x, start, B, H, **PAR), f"short pushes from {start}")


# ---------------------------------------------------------------- 4. strides
@pytest.mark.parametrize("i", [2, 6], ids=["time", "streams"])
def test_padded_strides_with_nan_in_the_gaps(i):
    K, B, H, _ = SHAPES[i]
    x, _ = _case(i)
    key = lr.noise(len(x), K, 99)
    want = lr.model_push(x, 0, B, H, key=key, **PAR)
    half = [len(x) // 2, len(x) - len(x) // 2]
    with _plan(K, B, H) as plan:
        equal(push_cut(plan, x, half, key=key, stride=K + 13, key_stride=K + 5), want, f"{IDS[i]} at strides K + 13, K + 5")
        plan.level_reset(0)
        equal(push_cut(plan, x, half, stride=K + 13), _case(i)[1], f"{IDS[i]} at stride K + 13, no key")


def test_lane_subsets_in_place():
    """64, 8 and 3 neighbouring lanes of a 64-wide array by pointer offset and the array's stride,
    against the columns of the model of all 64: the wave-wide streams form, the narrow one and the
    time form give the same bits."""
    B, H = 16, 5
    x = lr.noise(500, 64, 77)
    d_x = _dev(x)
    want = lr.model_push(x, 0, B, H, **PAR)
    kinds = {}
    for K, off in ((64, 0), (8, 24), (3, 41)):
        with _plan(K, B, H) as plan:
            f = level_form(plan.lib, K, B, H, 0, 0, 500)
            kinds[K] = (f["kind"], f["lanes"])
            r = np.concatenate([_push_ptr(plan, d_x.data_ptr() + 4 * off, 203, 64),
                                _push_ptr(plan, d_x.data_ptr() + 4 * (203 * 64 + off), 297, 64)])
        equal(r, want[:, off:off + K], f"{K} lanes at {off}")
    assert kinds == {64: (lr.STREAMS, 64), 8: (lr.STREAMS, 8), 3: (lr.TIME, 3)}


def test_a_stride_that_puts_the_last_sample_past_4_gib():
    import torch
    K, B, H, n, stride = 8, 8, 1, 70, 1 << 24
    assert (n - 1) * stride * 4 > 2 ** 32
    x = lr.noise(n, K, 88)
    try:
        d_x = torch.empty(((n - 1) * stride + K,), dtype=torch.float32, device="cuda")
    except torch.cuda.OutOfMemoryError:
        pytest.skip("no 4.4 GiB of device memory for the input")
    d_x.as_strided((n, K), (stride, 1)).copy_(_dev(x))    # laid out on the device
    with _plan(K, B, H) as plan:
        r = np.concatenate([_push_ptr(plan, d_x.data_ptr(), 33, stride), _push_ptr(plan, d_x.data_ptr() + 4 * 33 * stride, n - 33, stride)])
    equal(r, lr.model_push(x, 0, B, H, **PAR), "stride 2^24")


# ---------------------------------------------------------------- 5. the key
@pytest.mark.parametrize("K,B,H", [(16, 16, 2), (3, 16, 2)], ids=["streams", "time"])
def test_the_gains_follow_the_key_and_x_changes_nothing_but_the_product(K, B, H):
    n = 20 * B + 5
    x, key = lr.noise(n, K, 41, lo_db=-20.0), lr.noise(n, K, 42)
    cut = [3 * B + 1, 1, n - 3 * B - 2]
    with _plan(K, B, H) as plan:
        a = push_cut(plan, x, cut, key=key)
        plan.level_reset(0)
        b = push_cut(plan, np.float32(2.0) * x, cut, key=key)     # another x under the same key: twice the output, exactly
        plan.level_reset(0)
        own = push_cut(plan, x, cut)
    equal(a, lr.model_push(x, 0, B, H, key=key, **PAR), "keyed")
    assert not lr.same(a, own) and lr.same(own, lr.model_push(x, 0, B, H, **PAR))
    assert np.isfinite(a).all() and b.tobytes() == (np.float32(2.0) * a).tobytes()
    assert np.abs(a).max() > 0.5 * 1.01                           # the key's level, not x's: the target does not bind x


# ---------------------------------------------------------------- 6. NaN and inf
@pytest.mark.parametrize("K,B,H", [(16, 8, 2), (3, 8, 2)], ids=["streams", "time"])
def test_a_nan_or_an_inf_stays_in_its_lane(K, B, H):
    n = 16 * B + 3
    base_x = lr.noise(n, K, 19, lo_db=-40.0)
    p = 5 * B + B - 1                                     # the last step of a block
    base_x[p] = 0.0                                       # (not its block's peak: m(NaN) = 0 then moves no peak)
    with _plan(K, B, H) as plan:
        base = _push(plan, base_x)
        for s in (0, K - 1):
            for bad in (np.nan, np.inf, -np.inf):
                x = base_x.copy()
                x[p, s] = bad
                plan.level_reset(0)
                r = push_cut(plan, x, [p + 1, n - p - 1])  # the bad sample goes through the carry
                others = np.arange(K) != s
                assert r[:, others].tobytes() == base[:, others].tobytes(), f"the other lanes, {bad} in lane {s}"
                with np.errstate(all="ignore"):
                    want = lr.model_push(x[:, s:s + 1], 0, B, H, **PAR)
                equal(r[:, s:s + 1], want, f"lane {s} with its {bad}")
                changed = np.nonzero(r[:, s].view(np.uint32) != base[:, s].view(np.uint32))[0]
                if np.isnan(bad):                         # m(NaN) = 0: the NaN itself and nothing else
                    assert changed.tolist() == [p] and np.isnan(r[p, s])
                else:                                     # 2^60 in the peaks of blocks 5 .. 5 + H: the ramps around them
                    assert changed.min() >= 4 * B and changed.max() < (5 + H + 2) * B and not np.isfinite(r[p, s])


# ---------------------------------------------------------------- 7. more tiles than the grid
def test_more_tiles_than_workgroups():
    """The smallest shape whose tiles pass the grid's 4096: 2048 lanes are 32 lane tiles of 64, a
    tile is 256 steps at B = 8, so 129 spans of steps.  Whole lanes against the model: the first and
    last of a lane tile, of the first, a middle and the last tile."""
    import torch
    K, B, H = 2048, 8, 3
    n = 129 * 256 + 2 * B + 5
    with _plan(K, B, H) as plan:
        f = level_form(plan.lib, K, B, H, 0, 0, n)
        assert (f["lanes"], f["rows"], f["lane_tiles"]) == (64, 256, 32)
        assert f["p_tiles"] > f["p_grid"] == 1 << 12 and f["a_tiles"] > f["a_grid"] == 1 << 12
        picks = [0, 63, 64, 1000, 1023, 1984, 2047]
        scale = 10.0 ** (-4.0 * np.random.default_rng(6).uniform(0.0, 1.0, (n // 40 + 1, 1)))
        x = (np.random.default_rng(5).uniform(-1.0, 1.0, (n, K)) * np.repeat(scale, 40, axis=0)[:n]).astype(np.float32)
        d_x = _dev(x)
        outs = plan.level_steps(n)
        d_r = stall.sentinel((outs * K + 64,))
        plan.level_push_device(d_x.data_ptr(), n, K, d_r.data_ptr())
        torch.cuda.synchronize()
        assert (d_r[outs * K:] == stall.SENTINEL).all().item()
        r = d_r[:outs * K].view(outs, K)[:, picks].cpu().numpy()
        env, gain = plan.level_meter()
    equal(r, lr.model_push(np.ascontiguousarray(x[:, picks]), 0, B, H, **PAR), "lanes of three lane tiles")
    E, G = lr.meter(np.ascontiguousarray(x[:, picks]), 0, B, H, **PAR)
    equal(env[picks], E, "envelope")
    equal(gain[picks], G, "gain")


# ---------------------------------------------------------------- 8. the meter
@pytest.mark.parametrize("K,B,H", [(9, 8, 4), (2, 8, 4)], ids=["streams", "time"])
def test_the_meter_is_the_newest_complete_block(K, B, H):
    cut = [3, B - 4, 1, 2 * B, 1, B - 1, 5 * B + 2, 1, 7 * B]
    x, key = lr.noise(sum(cut), K, 71), lr.noise(sum(cut), K, 72)
    for start in (0, 2 ** 32 - 100):
        with _plan(K, B, H) as plan:
            plan.level_reset(start)
            E, G = plan.level_meter()
            assert (E == 0).all() and lr.same(G, lr.meter(key[:0], start, B, H, **PAR)[1]) and (G == 0).all()
            at = 0
            for c in cut:
                _push(plan, x[at:at + c], key[at:at + c])
                at += c
                E, G = plan.level_meter()
                wE, wG = lr.meter(key[:at], start, B, H, **PAR)
                equal(E, wE, f"envelope after {at} steps from {start}")
                equal(G, wG, f"gain after {at} steps from {start}")
        assert (wG > 0).any()
    with _plan(K, B, H, squelch=0.0) as plan:             # no squelch: E = 0 gives gmax
        assert (plan.level_meter()[1] == np.float32(PAR["gmax"])).all()


# ---------------------------------------------------------------- 9. ordering
@pytest.mark.parametrize("reset", [False, True], ids=["push", "reset-between"])
def test_a_device_push_behind_a_stalled_stream(reset):
    """demod_push_device on A and, right after it, a level push on B that reads its output and
    another on C, enqueued while a bounded spin kernel holds A (tests/stall.py), then a synchronous
    host push behind them: nothing runs ahead of the plan's earlier work and the results equal the
    stepped run's bytewise -- also with a level_reset enqueued between the two device pushes."""
    import torch
    import demod_ref as dr
    from pypanadapter_amd import ZoomFFT
    streams = stall.streams()
    K, Ta, Da, B, H = 16, 33, 4, 16, 3
    x = dr.noise_and_tones(3000, K, 37)
    g = dr.audio_taps(Ta, Da)
    tail = lr.noise(200, K, 5)
    na = dr.steps(0, 3000, Da)
    n1 = 401
    par = dict(PAR, squelch=0.0)

    def bufs():
        return {"x": torch.from_numpy(x.view(np.float32).reshape(-1, 2).copy()).to("cuda"), "a": stall.sentinel((na * K,)),
                "r": stall.sentinel((na * K,))}

    def seq(plan, run, b):
        run.call("demod_push", plan.demod_push_device, b["x"].data_ptr(), 3000, K, 1, b["a"].data_ptr(), on=streams[0])
        o1 = plan.level_steps(n1)
        run.call("level_push0", plan.level_push_device, b["a"].data_ptr(), n1, K, b["r"].data_ptr(), on=streams[1])
        if reset:
            run.host(plan.level_reset, n1)
        run.call("level_push1", plan.level_push_device, b["a"].data_ptr() + 4 * n1 * K, na - n1, K,
                 b["r"].data_ptr() + 4 * o1 * K, on=streams[2])

    def make():
        plan = ZoomFFT(32, 1, 1.0)
        plan.set_demod(K, taps=g, decim=Da)
        plan.set_level(K, B, H, **par)
        seq(plan, stall.Run(plan, streams, held=False), bufs())   # the workspaces have their size
        plan.level_push(tail)
        torch.cuda.synchronize()
        plan.demod_reset(0)
        plan.level_reset(0)
        torch.cuda.synchronize()
        return plan, bufs()

    def sequence(plan, run, b):
        seq(plan, run, b)
        run.check_order()
        if run.held:
            assert stall.quiesce_count(plan) == run.q0            # no host wait in any enqueue, the reset's included
        after = run.waiting("level_push_host", plan.level_push, tail)
        return {"a": b["a"], "r": b["r"], "after": after, "steps": plan.level_state()}

    held, stepped, run = stall.enqueue_twice(f"level[{'reset' if reset else 'push'}]", make, sequence, streams)
    stall.same_bytes(held, stepped, "held")
    a = held["a"].reshape(na, K)
    assert not (a == stall.SENTINEL).any()
    if reset:                                                     # the second push starts again, at count n1, from a zero past
        o1 = lr.steps(0, 0, n1, B)
        first, second = lr.model_push(a[:n1], 0, B, H, **par), lr.model_push(np.concatenate([a[n1:], tail]), n1, B, H, **par)
        want = np.concatenate([first, second[:lr.steps(n1, n1, na - n1, B)]])
        after = second[lr.steps(n1, n1, na - n1, B):]
        assert len(first) == o1
    else:
        whole = lr.model_push(np.concatenate([a, tail]), 0, B, H, **par)
        want, after = whole[:lr.steps(0, 0, na, B)], whole[lr.steps(0, 0, na, B):]
    assert held["steps"] == na + len(tail)
    equal(held["r"][:want.size].reshape(want.shape), want, "the two pushes behind the held stream")
    assert (held["r"][want.size:] == stall.SENTINEL).all()
    equal(held["after"], after, "the host push behind them")


# ---------------------------------------------------------------- 10. end to end
def test_end_to_end_channeliser_demodulator_level_resampler():
    """An AM carrier with 50 % tone modulation in one channel of a (64, 8, 32) bank at 2.4 MHz, its
    amplitude stepping down by 40 dB, and weak noise alone in another channel: Channelizer ->
    Demodulator("am", audio_decim=4) -> LevelControl -> Resampler(48 kHz, "s16").  The level bank's
    output is level_ref's model of the audio and the PCM resamp_ref's of that, bit for bit.

    The control, without the level bank: the quiet stretch's codes peak 40 dB below the loud one's.
    With it, the peaks of the two stretches, each from H + 2 blocks after the step on, agree within

        1 + 32767 target (S (d_loud + d_quiet + 2^-20) + 2 (rho + leak))   codes:

    the tone's period (16 audio steps) divides the block, so every block of a stretch has the same
    peak but for d, the spread of the audio's own block peaks there (measured on the bank's input);
    then E is that peak, the gain target / E within rule 6's 2^-21, and the two stretches leave the
    bank as the same waveform at level `target` but for d_loud + d_quiet + 2 x 2^-21.  The resampler
    multiplies a difference of bounded inputs by at most S = max over phases of sum |h|; its ripple
    rho at the tone and the leaking images move a peak of either stretch by (rho + leak) target, and
    each code is rounded by half a code."""
    import resamp_ref as rr
    from test_gpu_resamp import _tone_bound
    from pypanadapter_amd import Channelizer, Demodulator, LevelControl, Resampler, resamp_design
    fs, Mc, D, Da, c, c_noise = 2.4e6, 64, 32, 4, 5, 20
    f_a = 1.0 / 16                                        # the tone, cycles per audio step
    n_a = 2 * 6400                                        # audio steps: two stretches
    n = n_a * Da * D
    t = np.arange(n, dtype=np.float64)
    # (the onset and the step are raised-cosine ramps of 2048 samples, so that neither splatters into the noise lane)
    ramp = lambda at: 0.5 - 0.5 * np.cos(np.pi * np.clip((t - at) / 2048.0, 0.0, 1.0))
    amp = 0.3 * ramp(0) - 0.297 * ramp(n // 2)
    rng = np.random.default_rng(3)
    x = amp * (1 + 0.5 * np.cos(2 * np.pi * (f_a / (Da * D)) * t)) * np.exp(2j * np.pi * (c / Mc) * t)
    x = x + 1e-5 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.exp(2j * np.pi * (c_noise / Mc) * t) * 0.1
    x = x.astype(np.complex64)
    target, squelch = 0.5, 1e-4
    bank = Channelizer(fs, Mc, ascending=False)
    try:
        audio = Demodulator.for_channelizer(bank, "am", audio_decim=Da)
        a = audio.push(bank.push(x))
        assert audio.rate == 18750.0 and a.shape == (n_a, Mc)
        plain = Resampler.for_demodulator(audio, 48e3, format="s16")
        q0 = plain.push(a)
        plain.close()
        level = LevelControl.for_demodulator(audio, target=target, attack_s=64 / 18750.0, hold_s=0.25, squelch=squelch)
        B, H = level.block, level.hold
        assert (B, H) == (64, 74) and level.latency == (64.0, 127.0)
        assert bank._plan.level_shape()[:3] == (Mc, B, H)
        pcm = Resampler.for_level(level, 48e3, format="s16")
        assert (pcm.L, pcm.M, pcm.lanes, pcm.rate) == (64, 25, Mc, 48e3)
        y = np.concatenate([level.push(a[:5001]), level.push(a[5001:])])
        q = pcm.push(y)
        met = level.meter()
        par = dict(target=target, gmax=1e4, floor=1e-6, squelch=squelch)
        equal(y, lr.model_push(a, 0, B, H, **par), "the level bank against the model of its own input")
        h = resamp_design(64, 25).astype(np.float32)
        equal(q, rr.quantise(rr.model_push(y, 0, h, 64, 25)), "int16 PCM at 48 kHz")
        # the windows: from H + 2 blocks after the start and after the step, to the step and the end
        half = n_a // 2
        w_l, w_q = slice((H + 2) * B, half - 2 * B), slice(half + (H + 2) * B, len(y) - 2 * B)
        to_out = lambda s: slice(s.start * 64 // 25 + 64, s.stop * 64 // 25 - 64)      # (the prototype's length inside)
        peak = lambda v, s: float(np.abs(v[to_out(s), c].astype(np.float64)).max())
        # the control
        ratio_db = 20 * np.log10(peak(q0, w_l) / peak(q0, w_q))
        print(f"without the bank: code peaks {peak(q0, w_l):.0f} and {peak(q0, w_q):.0f}, {ratio_db:.2f} dB apart")
        assert abs(ratio_db - 40.0) < 0.5 and peak(q0, w_q) < 200
        # the bound
        def spread(s):
            P = np.abs(a[s, c]).reshape(-1, B).max(axis=1)
            return float(P.max() / P.min() - 1.0)
        S = float(np.abs(h.astype(np.float64)).reshape(-1, 64).sum(axis=0).max())
        ripple = _tone_bound(h, 64, f_a, 1.0, real=True)[0]
        bound = 1 + 32767 * target * (S * (spread(w_l) + spread(w_q) + 2.0 ** -20) + 2 * ripple)
        p_l, p_q = peak(q, w_l), peak(q, w_q)
        print(f"with it: code peaks {p_l:.0f} and {p_q:.0f}: |diff| {abs(p_l - p_q):.1f} of {bound:.1f} "
              f"(spreads {spread(w_l):.2e}, {spread(w_q):.2e}, S {S:.3f}, ripple {ripple:.2e})")
        assert abs(p_l - p_q) <= bound < 0.01 * 32767 * target
        assert 0.9 * 32767 * target < p_q and np.abs(q.astype(np.int32)).max() < 32767 and q.min() > -32768      # no code on a rail
        # the noise lane stays closed
        assert (q[:, c_noise] == 0).all() and (y[:, c_noise] == 0).all() and np.abs(a[:, c_noise]).max() > 0
        assert not met["open"][c_noise] and met["open"][c] and met["gain"][c_noise] == 0
        assert met["envelope"][c] == np.abs(a[-(len(a) % B) - (H + 1) * B:len(a) - len(a) % B, c]).max()
    finally:
        bank.close()


# ---------------------------------------------------------------- 11. off means off; calls and errors
def test_off_means_off():
    from pypanadapter_amd import ZoomFFT, synth
    x = np.stack([synth.make_iq(65536, 2.4e6, 3 + f, n_fft=1024, zoom=8, n_win=128) for f in range(16)])
    y = lr.noise(500, 4, 3)
    with ZoomFFT(1024, 8, 2.4e6, n_win=128) as plan:
        plan.set_timing(True)
        rows = plan.rows(x)
        names = plan.launch_names()
        assert names and not [n for n in names if "level" in n]

        def off():
            assert plan.lib.zfft_level_shape is not None
            for call in (plan.level_state, plan.level_shape, lambda: plan.level_steps(5), lambda: plan.level_push(y),
                         plan.level_info, plan.level_reset, plan.level_meter, lambda: plan.level_push_device(8, 1, 4, 8)):
                with pytest.raises(ValueError, match="level is off"):
                    call()
        off()
        plan.set_level(4, 8, 2)                           # on: a process call is still the plan's alone
        assert plan.level_shape()[:3] == (4, 8, 2)
        assert np.array_equal(plan.rows(x), rows) and plan.launch_names() == names
        r = plan.level_push(y)
        assert plan.launch_names() == ["level_peaks", "level_gains", "level_apply"] and len(plan.timings()) == 3
        assert r.shape == (500 // 8 * 8 - 8, 4)
        assert plan.level_push(y[:3]).shape == (0, 4) and plan.launch_names() == ["level_peaks", "level_apply"]
        plan.set_level(0)                                 # off again, everything freed
        off()
        assert np.array_equal(plan.rows(x), rows) and plan.launch_names() == names
        plan.set_level(0)


def test_calls_and_errors():
    from pypanadapter_amd import ZoomFFT, _lib
    with ZoomFFT(32, 1, 1.0) as plan:
        ok = (4, 8, 2, 0.5, 1e4, 1e-6, 0.0)
        for at, bad in [(0, -1), (0, 2049), (1, 4), (1, 12), (1, 2048), (1, 0), (2, -1), (2, 4097), (3, 0.0), (3, 2.0 ** 61),
                        (3, float("nan")), (4, 2.0 ** -61), (4, float("inf")), (5, 0.0), (5, -1.0), (6, -1.0), (6, 2.0 ** -61),
                        (6, float("nan"))]:
            args = list(ok)
            args[at] = bad
            assert plan.lib.zfft_plan_level(plan._plan, *args) == _lib.ZFFT_EINVAL, (at, bad)
        assert b"level" in plan.lib.zfft_last_error()
        with pytest.raises(ValueError, match="level is off"):
            plan.level_state()                            # a refused call enables nothing
        plan.set_level(3, 8, 0, target=2.0 ** 60, gmax=2.0 ** -60, floor=2.0 ** 60, squelch=2.0 ** 60)   # the limits themselves
        assert plan.level_shape() == (3, 8, 0, 2.0 ** 60, 2.0 ** -60, 2.0 ** 60, 2.0 ** 60) and plan.level_state() == 0
        d = _dev(np.zeros((16, 3)))
        o = _dev(np.zeros((16, 3)))
        p, r = d.data_ptr(), o.data_ptr()
        for bad in [(p, 16, 2, r), (p, 16, 2 ** 31 + 1, r), (0, 16, 3, r), (p + 2, 16, 3, r), (p, 16, 3, r + 1), (p, -1, 3, r),
                    (p, 2 ** 31, 3, r), (p, 16, 3, 0), (p, 16, 3, p), (p, 16, 3, r, p, 2), (p, 16, 3, r, p + 2, 3), (p, 16, 3, r, r, 3)]:
            with pytest.raises(ValueError, match="level"):
                plan.level_push_device(*bad)
        assert plan.level_state() == 0
        with pytest.raises(ValueError, match="n0 in"):
            plan.level_reset(2 ** 62 + 1)
        plan.level_reset(2 ** 62 - 3)
        with pytest.raises(ValueError, match="count would pass"):
            plan.level_push(np.zeros((4, 3), np.float32))
        assert plan.level_push(np.zeros((3, 3), np.float32)).shape == (0, 3) and plan.level_state() == 2 ** 62
        with pytest.raises(ValueError, match="key"):
            plan.level_push(np.zeros((3, 3), np.float32), key=np.zeros((2, 3), np.float32))
        # one lane, 1-D, with a key: the gain is the fixed gmax wherever the key opens the squelch
        plan.set_level(1, 8, 0, target=2.0 ** 60, gmax=3.0, floor=1e-6, squelch=0.5)
        x = lr.noise(64, 1, 1)[:, 0]
        key = np.repeat(np.float32([1, 1, 1, 0, 0, 0, 1, 1]), 8)
        out = plan.level_push(x, key=key)
        equal(out, lr.model_push(x[:, None], 0, 8, 0, key=key[:, None], target=2.0 ** 60, gmax=3.0, floor=1e-6, squelch=0.5), "1-D")
        assert (out[24:40] == 0).all() and out[8:16, 0].tobytes() == (np.float32(3.0) * x[8:16]).tobytes()
