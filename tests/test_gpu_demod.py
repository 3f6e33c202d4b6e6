"""GPU checks of the demodulator bank (zfft_plan_demod; csrc/demod_kernels.hip) against
tests/demod_ref.py, the rule of include/zfft.h in numpy float64.  The error gate is the header's
rule 6 (demod_ref.gate): (Ta + 32) 2^-24 sum|g| max|d| + sum|g| eps_mode, eps derived for AM, SSB
and POWER; FM's is EPS_FM 2^-24, twice the worst detector error the first run on an MI355X
measured, rounded up, under the condition EPS_FM <= 16 (test_detector_errors prints the figure).
Every comparison prints its worst ratio to the gate before it asserts.

Figures of the first run on an MI355X (worst |a - ref| / gate per test, the detector errors) are in
profiles/demod/README.md."""
import ctypes
import functools

import numpy as np
import pytest

import demod_ref as dr
import stall
import tap_ref as tp

pytestmark = pytest.mark.gpu
MODE_NAMES = ["am", "fm", "ssb", "power"]


@pytest.fixture(scope="module", autouse=True)
def _gpu(zfft_lib):
    from pypanadapter_amd import device_count
    assert device_count() >= 1, "GPU tests need a HIP device"


def _plan(K, Ta, Da, g=None, modes=None, words=None):
    """A plan with the bank on; modes / words per stream (default: all AM)."""
    from pypanadapter_amd import ZoomFFT
    plan = ZoomFFT(32, 1, 1.0)
    plan.set_demod(K, taps=g, decim=Da)
    assert plan.demod_shape() == (K, Ta, Da)
    if modes is not None:
        _set_modes(plan, modes, words)
    return plan


def _set_modes(plan, modes, words=None):
    K = plan.demod_shape()[0]
    modes = np.broadcast_to(np.asarray(modes), (K,))
    words = np.broadcast_to(np.asarray(0 if words is None else words, dtype=np.int64), (K,))
    s = 0
    while s < K:                                       # runs of equal parameters: one call each
        e = s
        while e < K and modes[e] == modes[s] and words[e] == words[s]:
            e += 1
        used = plan.demod_mode(int(modes[s]), bfo_hz=int(words[s]) / 2.0 ** 32, first=s, count=e - s)   # (fs = 1)
        assert used == int(words[s]) / 2.0 ** 32
        s = e


def _form(plan, layout, n0=0, n=1):
    from test_demod_host import demod_form
    K, Ta, Da = plan.demod_shape()
    return demod_form(plan.lib, K, Ta, Da, *dr.strides(layout, K, max(n, 2)), n0, n)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.complex64).view(np.float32).reshape(-1, 2).copy()).to("cuda")


def _push(plan, x, layout="streams"):
    """One device push of the (steps, K) array laid out as `layout`; (outputs, K) float32.  Nothing
    beyond outputs x K is written."""
    import torch
    n, K = x.shape
    ss, ts = dr.strides(layout, K, n)
    outs, guard = plan.demod_steps(n), 64
    d_x = _dev(dr.lay(x, layout))
    d_a = stall.sentinel((outs * K + guard,))
    plan.demod_push_device(d_x.data_ptr(), n, ss, ts, d_a.data_ptr())
    torch.cuda.synchronize()
    a = d_a.cpu().numpy()
    assert (a[outs * K:] == stall.SENTINEL).all()
    return a[:outs * K].reshape(outs, K).copy()


def _under(got, ref, bounds, what):
    """max over streams of |a - ref| / gate; bounds a scalar or one per stream."""
    bounds = np.broadcast_to(np.asarray(bounds, dtype=np.float64), (ref.shape[1],))
    err = np.abs(got.astype(np.float64) - ref) if ref.size else np.zeros((1, ref.shape[1]))
    ratio = float((err.max(axis=0) / bounds).max())
    print(f"{what}: max|a - ref| = {float(err.max()):.3e}, worst ratio to the gate {ratio:.4f}")
    assert got.shape == ref.shape and got.dtype == np.float32 and ratio <= 1.0, (what, ratio)
    return ratio


@functools.lru_cache(maxsize=None)
def _signal(i, fm, n):
    """Case i's input, (n, K) complex64: constant-envelope FM, or noise and tones.  Read-only."""
    K = dr.CASES[i][0]
    x = dr.fm_signal(n, K, dr.fm_seed(i)) if fm else dr.noise_and_tones(n, K, 7 + i)
    x.setflags(write=False)
    return x


def _words(K, seed):
    return np.random.default_rng(seed).integers(-2 ** 31, 2 ** 31, K)


# ---------------------------------------------------------------- 1. every case, every mode
@pytest.mark.parametrize("mode", MODE_NAMES)
@pytest.mark.parametrize("i", range(len(dr.CASES)), ids=dr.IDS)
def test_each_mode_under_the_derived_gate(i, mode):
    K, Ta, Da, layout = dr.CASES[i]
    m = dr.MODES[mode]
    g = dr.audio_taps(Ta, Da)
    words = _words(K, 100 + i) if m == dr.SSB else np.zeros(K, np.int64)
    with _plan(K, Ta, Da, g, m, words) as plan:
        f = _form(plan, layout)
        n = dr.case_len(f["span"])
        f = _form(plan, layout, 0, n)
        assert f["nspans"] >= 4 and n % f["span"] and f["ntiles"] >= 3 * f["stream_tiles"]   # three tiles and a ragged tail
        assert f["kind"] == (1 if layout == "streams" and K >= 8 else 0)
        x = _signal(i, m == dr.FM, n)
        if m == dr.FM:
            assert dr.fm_arg_ok(x)                      # the bound's condition, on the reference, before any comparison
        assert plan.demod_info() == {"group_delay": (Ta - 1) / 2, "rate_ratio": 1.0 / Da}
        a = _push(plan, x, layout)
        assert plan.demod_state() == n
    ref = dr.ref_push(x, 0, m, words, g, Da)
    _under(a, ref, dr.gate(g, m, np.abs(x).max()), f"{dr.IDS[i]} {mode}")


# ---------------------------------------------------------------- 2. the detectors alone
def test_detector_errors():
    """Ta = 1, g = [1], Da = 1: a = fma(1, d, 0) = d, the detected value itself.  Prints the worst
    |d - d_ref| of every mode in units of 2^-24 (FM's is the figure EPS_FM is set from) and asserts
    each under its eps."""
    K, n = 64, 4096
    g = np.float32([1.0])
    worst = {}
    for mode in MODE_NAMES:
        m = dr.MODES[mode]
        x = dr.fm_signal(n, K, 31) if m == dr.FM else dr.noise_and_tones(n, K, 41)
        if m == dr.FM:
            assert dr.fm_arg_ok(x)
        words = _words(K, 5) if m == dr.SSB else np.zeros(K, np.int64)
        with _plan(K, 1, 1, g, m, words) as plan:
            d = _push(plan, x)
        ref = dr.detect(x, 0, m, words)
        err = float(np.abs(d.astype(np.float64) - ref).max())
        worst[mode] = err / dr.U
        print(f"detector {mode}: worst |d - d_ref| = {err:.3e} = {err / dr.U:.3f} x 2^-24 (eps {dr.eps(m, np.abs(x).max()) / dr.U:.2f} x 2^-24)")
        assert d.shape == ref.shape and err <= dr.eps(m, np.abs(x).max()), (mode, err)
    assert worst["fm"] <= dr.EPS_FM <= 16


# ---------------------------------------------------------------- 3. cut invariance, one case per form
@pytest.mark.parametrize("i", [4, 1], ids=[dr.IDS[4], dr.IDS[1]])
def test_outputs_do_not_depend_on_the_cut_bit_for_bit(i):
    K, Ta, Da, layout = dr.CASES[i]
    g = dr.audio_taps(Ta, Da)
    rng = np.random.default_rng(50 + i)
    for modes in ([np.arange(K) % 4] if K > 1 else [[m] for m in range(4)]):
        words = _words(K, 60 + i)
        with _plan(K, Ta, Da, g, modes, words) as plan:
            span = _form(plan, layout)["span"]
            cut = [1, 1, 7, max(Da - 1, 1), max(Ta - 2, 1), Ta - 1 or 1, Ta, span - 1, span + 1] + rng.integers(1, 2 * span, 4).tolist()
            n = sum(cut) + 2 * span + 5
            cut.append(n - sum(cut))
            x = dr.fm_signal(n, K, 33 if K == 1 else 34)       # (constant envelope: every detector has work)
            whole = _push(plan, x, layout)
            assert plan.demod_state() == n
            plan.demod_reset(0)
            parts, at = [], 0
            for c in cut:
                want = plan.demod_steps(c)
                assert want == dr.steps(at, c, Da)
                parts.append(_push(plan, x[at:at + c], layout))
                assert parts[-1].shape == (want, K)
                at += c
            assert plan.demod_state() == n
        parts = np.concatenate(parts)
        assert min(cut) == 1 and any(c < Ta for c in cut)      # cuts of one step and cuts shorter than the carry
        assert parts.shape == whole.shape == (dr.steps(0, n, Da), K)
        assert parts.tobytes() == whole.tobytes()


# ---------------------------------------------------------------- 4. form independence
def test_both_forms_give_the_same_bits():
    K, Ta, Da = 64, 65, 8
    g = dr.audio_taps(Ta, Da)
    modes, words = np.arange(K) % 4, _words(K, 70)
    x = dr.fm_signal(1500, K, 35)
    with _plan(K, Ta, Da, g, modes, words) as plan:
        assert _form(plan, "streams")["kind"] == 1 and _form(plan, "time")["kind"] == 0
        a = _push(plan, x[:700], "streams")
        b = _push(plan, x[700:], "time")               # the carry goes from one form to the other
        plan.demod_reset(0)
        c = _push(plan, x[:333], "time")
        d = _push(plan, x[333:], "streams")
    assert np.concatenate([a, b]).tobytes() == np.concatenate([c, d]).tobytes()
    ref = dr.ref_push(x, 0, modes, words, g, Da)
    _under(np.concatenate([a, b]), ref, dr.gates(g, modes, np.abs(x).max()), "forms")


# ---------------------------------------------------------------- 5. mixed modes, a change between pushes
def test_mixed_modes_in_one_wave_and_a_change_between_pushes():
    K, Ta, Da = 64, 33, 4
    g = dr.audio_taps(Ta, Da)
    rng = np.random.default_rng(80)
    modes, words = rng.integers(0, 4, K), _words(K, 81)
    assert len(set(modes.tolist())) == 4
    x = dr.fm_signal(3000, K, 32)
    assert dr.fm_arg_ok(x)
    n1 = 1777
    later = (modes + 1 + rng.integers(0, 3, K)) % 4     # every stream changes its mode
    assert (later != modes).all()
    with _plan(K, Ta, Da, g, modes, words) as plan:
        a = _push(plan, x[:n1])
        _set_modes(plan, later, words)
        b = _push(plan, x[n1:])
    xmax = np.abs(x).max()
    _under(a, dr.ref_push(x[:n1], 0, modes, words, g, Da), dr.gates(g, modes, xmax), "mixed modes")
    # the new mode applies to the carried window: the reference detects the whole stream with it
    ms = dr.step_indices(n1, len(x) - n1, Da)
    _under(b, dr.ref_demod(x, 0, later, words, g, Da, ms), dr.gates(g, later, xmax), "after the change")


# ---------------------------------------------------------------- 6. impulses
@pytest.mark.parametrize("layout", ["streams", "time"])
def test_impulses_give_exact_zeros_outside_their_window(layout):
    K, Ta, Da, A = 8, 17, 3, 0.75
    g = dr.audio_taps(Ta, Da)
    modes, words = np.arange(K) % 4, _words(K, 90)
    with _plan(K, Ta, Da, g, modes, words) as plan:
        span = _form(plan, layout)["span"]
        pos = [span - 1, 2 * span, 2 * span + 5 * Ta + 1]      # the last step of a span, the first of another, one inside
        n = 3 * span + 11
        x = np.zeros((n, K), np.complex64)
        for j, p in enumerate(pos):
            x[p] = A * np.exp(2j * np.pi * (0.37 * j + 0.11 * np.arange(K)))
            x[p + 1, modes == dr.FM] = A * np.exp(1.3j)         # FM sees a pair: one non-zero product
        assert _form(plan, layout, 0, n)["nspans"] == 4
        a = _push(plan, x, layout)
    ref = dr.ref_push(x, 0, modes, words, g, Da)
    at = np.arange(a.shape[0]) * Da                           # output m is step m Da
    for s in range(K):
        w = Ta + 1 if modes[s] == dr.FM else Ta               # FM's window is one longer
        inside = np.zeros(a.shape[0], bool)
        for p in pos:
            inside |= (at >= p) & (at <= p + w - 1)
        assert inside.any() and not inside.all()
        assert not a[~inside, s].any() and not ref[~inside, s].any()      # exactly 0
        assert a[inside, s].any()
    # one non-zero term per output: sum|g| max|d| is max|g| max|d|
    gmax = float(np.abs(g).max())
    bound = np.array([(Ta + 32) * dr.U * gmax * dr.d_max(m, A) + gmax * dr.eps(m, A) for m in modes])
    _under(a, ref, bound, f"impulses {layout}")


# ---------------------------------------------------------------- 7. counts past 2^32
@pytest.mark.parametrize("n0", [2 ** 32 - 100, 2 ** 40 + 3])
def test_a_count_past_2_to_the_32(n0):
    K, Ta, Da = 8, 33, 8
    g = dr.audio_taps(Ta, Da)
    modes, words = np.array([dr.SSB] * 6 + [dr.FM, dr.AM]), _words(K, 95)
    x = dr.fm_signal(2000, K, 36)
    assert n0 % Da and dr.fm_arg_ok(x)
    for layout in ("streams", "time"):
        with _plan(K, Ta, Da, g, modes, words) as plan:
            plan.demod_reset(n0)
            assert plan.demod_state() == n0 and plan.demod_steps(777) == dr.steps(n0, 777, Da)
            a = _push(plan, x[:777], layout)
            b = _push(plan, x[777:], layout)
            assert plan.demod_state() == n0 + 2000
        _under(np.concatenate([a, b]), dr.ref_push(x, n0, modes, words, g, Da), dr.gates(g, modes, np.abs(x).max()),
               f"n0={n0} {layout}")


# ---------------------------------------------------------------- 8. ordering
def test_a_device_push_behind_a_stalled_stream():
    """process_device on A and, right after it, a bank push on B, a mode change and another push on
    C, enqueued while a bounded spin kernel holds A (tests/stall.py): nothing runs ahead of the
    plan's earlier work, no enqueue waits on the host, and both results are right."""
    import torch
    from pypanadapter_amd import ZoomFFT
    streams = stall.streams()
    F, L, N, K, Ta, Da = 4, 4096, 1024, 16, 33, 4
    iq = tp.noise_and_tones(F * L, 71)
    x = dr.fm_signal(3000, K, 37)
    assert dr.fm_arg_ok(x)
    g = dr.audio_taps(Ta, Da)
    n1 = 1501

    def bufs():
        return {"iq": torch.from_numpy(iq.view(np.float32).reshape(F, L, 2).copy()).to("cuda"), "x": _dev(x.reshape(-1)),
                "rows": stall.sentinel((F, N)), "a": stall.sentinel((dr.steps(0, 3000, Da) * K,))}

    def seq(plan, run, b):
        run.call("process", plan.process_device, b["iq"].data_ptr(), L, F, b["rows"].data_ptr(), on=streams[0])
        run.call("demod_push0", plan.demod_push_device, b["x"].data_ptr(), n1, K, 1, b["a"].data_ptr(), on=streams[1])
        run.host(plan.demod_mode, "fm")
        run.call("demod_push1", plan.demod_push_device, b["x"].data_ptr() + 8 * n1 * K, 3000 - n1, K, 1,
                 b["a"].data_ptr() + 4 * dr.steps(0, n1, Da) * K, on=streams[2])

    def make():
        plan = ZoomFFT(N, 1, 1.0)
        plan.set_demod(K, taps=g, decim=Da)
        seq(plan, stall.Run(plan, streams, held=False), bufs())   # the workspaces have their size
        torch.cuda.synchronize()
        plan.demod_mode("am")
        plan.demod_reset(0)
        torch.cuda.synchronize()
        return plan, bufs()

    def sequence(plan, run, b):
        seq(plan, run, b)
        run.check_order()
        return {"rows": b["rows"], "a": b["a"]}

    held, stepped, run = stall.enqueue_twice("demod[push]", make, sequence, streams)
    assert run.final_held and run.quiesce_delta == 0             # no host wait in any enqueue
    stall.same_bytes(held, stepped, "held")
    assert not (held["rows"] == stall.SENTINEL).any()
    a = held["a"].reshape(-1, K)
    o1 = dr.steps(0, n1, Da)
    xmax = np.abs(x).max()
    _under(a[:o1], dr.ref_push(x[:n1], 0, dr.AM, 0, g, Da), dr.gate(g, dr.AM, xmax), "the push before the change")
    _under(a[o1:], dr.ref_demod(x, 0, dr.FM, 0, g, Da, dr.step_indices(n1, 3000 - n1, Da)), dr.gate(g, dr.FM, xmax),
           "the push behind it")


# ---------------------------------------------------------------- 9. end to end on the device
def _tone(a, f, skip):
    """The amplitude of the real tone at f cycles per sample in a[skip:], by a heavy window."""
    s = a[skip:].astype(np.float64)
    w = np.blackman(s.size) * np.kaiser(s.size, 20.0)
    w /= w.sum()
    return 2.0 * abs(np.sum(w * s * np.exp(-2j * np.pi * f * np.arange(s.size))))


def _resp(h, nu):
    h = np.asarray(h, dtype=np.float64)
    return np.abs(np.exp(-2j * np.pi * np.outer(np.atleast_1d(nu), np.arange(h.size))) @ h)


FLOOR = 1e-6   # the window's leakage of the audio's DC term (-150 dB) and the input's float32 rounding


def _fm_slack(h, g, f_in, beta, amp, others):
    """What a prototype h that is not flat does to an FM tone's recovered amplitude: the lines k f_in,
    |k| <= 6, each off by at most rho = max||H| / H(0) - 1|, the lines beyond (Bessel tail) lost, and
    `others` = [(amplitude, offsets)] leaking in through the stopband; a relative perturbation delta of
    the channel's signal moves a phase by asin(delta), d by twice that over pi, the estimate by
    2 sum|g| of it."""
    from scipy.special import jv
    H0 = _resp(h, 0.0)[0]
    rho = np.abs(_resp(h, np.linspace(-6 * f_in, 6 * f_in, 97)) / H0 - 1.0).max()
    lines = sum(abs(jv(k, beta)) for k in range(-6, 7))
    tail = 2.0 * sum(abs(jv(k, beta)) for k in range(7, 40))
    leak = sum(A * _resp(h, nu).max() for A, nu in others) / (amp * H0)
    delta = rho * lines + tail + leak
    return 2.0 * np.abs(g).sum() * 2.0 * np.arcsin(delta) / np.pi, delta, lines, tail


def test_end_to_end_on_the_device_with_no_host_copy_between():
    """An FM and an AM carrier in two channels of a (64, 8, 32) bank: chan_push_device into a device
    buffer, demod_push_device out of it, nothing in between.  Each channel's audio is demod_ref of
    the bank's own output under the gate, and the recovered tones have the amplitudes the closed
    forms give -- FM: (2 beta / pi) sin(pi f_d) |G(f_d)| from d = (phase step) / pi of beta sin;
    AM: A mu H(0) |G(f_d)| -- within the gate plus what the prototype's passband ripple and
    stopband leakage, computed from g and h, can move them.  The same through one Tap."""
    import torch
    from pypanadapter_amd import ZoomFFT, chan_design, demod_design, tap_design
    M, P, D, Da = 64, 8, 32, 2
    c_fm, c_am, f_d = 5, 20, 0.01                       # f_d: the audio tone in cycles per channel step
    A1, beta, A2, mu = 0.5, 1.0, 0.1, 0.5
    warm, steps = 32, 2400                              # the bank's start-up (M P / D = 16 steps) runs first, on its own
    n0, n = warm * D, steps * D
    t = np.arange(n0 + n, dtype=np.float64)
    f_in = f_d / D
    x_fm = A1 * np.exp(1j * (2 * np.pi * (c_fm / M) * t + beta * np.sin(2 * np.pi * f_in * t)))
    x_am = A2 * (1 + mu * np.cos(2 * np.pi * f_in * t)) * np.exp(2j * np.pi * (c_am / M) * t)
    x = (x_fm + x_am).astype(np.complex64)
    h = chan_design(M, P).astype(np.float32)
    g = demod_design(8 * Da + 1, 0.4 / Da).astype(np.float32)
    G = _resp(g, f_d)[0]
    modes = np.zeros(M, np.int64)
    modes[c_fm] = dr.FM
    skip = g.size // Da + 8                             # past the audio filter's start
    d_x = _dev(x)
    with ZoomFFT(32, 1, 1.0) as plan:
        plan.set_channels(M, P, M // D, taps=h)
        plan.set_demod(M, decim=Da)                     # the default audio design
        plan.demod_mode("fm", first=c_fm, count=1)
        assert plan.chan_steps(n0) == warm and plan.demod_steps(steps) == steps // Da
        d_w = stall.sentinel((warm * M, 2))
        d_y = stall.sentinel((steps * M, 2))
        d_a = stall.sentinel((steps // Da * M,))
        plan.chan_push_device(d_x.data_ptr(), n0, d_w.data_ptr())
        plan.chan_push_device(d_x.data_ptr() + 8 * n0, n, d_y.data_ptr())
        plan.demod_push_device(d_y.data_ptr(), steps, M, 1, d_a.data_ptr())   # (K, 1): the bank's own layout
        torch.cuda.synchronize()
        y = np.ascontiguousarray(d_y.cpu().numpy()).view(np.complex64).reshape(steps, M)
        a = d_a.cpu().numpy().reshape(steps // Da, M)
    assert dr.fm_arg_ok(y[:, c_fm:c_fm + 1])
    _under(a, dr.ref_push(y, 0, modes, 0, g, Da), dr.gates(g, modes, np.abs(y).max()), "bank -> demod on the device")
    H0 = _resp(h, 0.0)[0]
    # FM
    got, want = _tone(a[:, c_fm], f_d * Da, skip), 2 * beta / np.pi * np.sin(np.pi * f_d) * G
    off = (c_am - c_fm) / M
    slack, delta, lines, tail = _fm_slack(h, g, f_in, beta, A1, [(A2 * (1 + mu), off + np.linspace(-f_in, f_in, 9))])
    bound = dr.gate(g, dr.FM, 1.0) + slack + FLOOR
    print(f"FM tone: {got:.7f} against {want:.7f} (delta {delta:.2e}): |diff| {abs(got - want):.2e} of {bound:.2e}")
    assert abs(got - want) <= bound and bound < 0.05 * want
    # AM
    got, want = _tone(a[:, c_am], f_d * Da, skip), A2 * mu * H0 * G
    ripple = A2 * mu * G * np.abs(_resp(h, [-f_in, f_in]) - H0).max()
    leak = A1 * (lines * _resp(h, -off + np.linspace(-6 * f_in, 6 * f_in, 97)).max() + tail * H0)   # the FM carrier's lines in this channel's stopband
    bound = dr.gate(g, dr.AM, np.abs(y[:, c_am]).max()) + ripple + 2 * np.abs(g).sum() * leak + FLOOR
    print(f"AM tone: {got:.7f} against {want:.7f}: |diff| {abs(got - want):.2e} of {bound:.2e}")
    assert abs(got - want) <= bound and bound < 0.01 * want
    # the same FM carrier through one tap, its output handed over on the device as (1, anything)
    T = 8 * D + 1
    ht = tap_design(T, 0.4 / D).astype(np.float32)
    with ZoomFFT(32, 1, 1.0) as plan:
        plan.set_taps(1, T)
        plan.tap_open(0, c_fm / M, D, taps=ht)
        plan.set_demod(1, decim=Da)
        plan.demod_mode("fm")
        assert int(plan.tap_counts(n0)[0]) == warm
        cnt = steps
        d_w = stall.sentinel((warm, 2))
        d_t = stall.sentinel((cnt, 2))
        d_a = stall.sentinel((cnt // Da,))
        plan.tap_push_device(d_x.data_ptr(), n0, d_w.data_ptr())
        assert int(plan.tap_counts(n)[0]) == cnt
        plan.tap_push_device(d_x.data_ptr() + 8 * n0, n, d_t.data_ptr())
        plan.demod_push_device(d_t.data_ptr(), cnt, 1, 0, d_a.data_ptr())
        torch.cuda.synchronize()
        yt = np.ascontiguousarray(d_t.cpu().numpy()).view(np.complex64).reshape(cnt, 1)
        at = d_a.cpu().numpy().reshape(cnt // Da, 1)
    assert dr.fm_arg_ok(yt)
    _under(at, dr.ref_push(yt, 0, dr.FM, 0, g, Da), dr.gate(g, dr.FM, np.abs(yt).max()), "tap -> demod on the device")
    got, want = _tone(at[:, 0], f_d * Da, skip), 2 * beta / np.pi * np.sin(np.pi * f_d) * G
    slack, delta, _, _ = _fm_slack(ht, g, f_in, beta, A1, [(A2 * (1 + mu), off + np.linspace(-f_in, f_in, 9))])
    bound = dr.gate(g, dr.FM, 1.0) + slack + FLOOR
    print(f"FM tone through a tap: {got:.7f} against {want:.7f} (delta {delta:.2e}): |diff| {abs(got - want):.2e} of {bound:.2e}")
    assert abs(got - want) <= bound and bound < 0.05 * want


def test_demodulator_wrappers():
    """Demodulator.for_channelizer and for_tap: what the sources push, as audio at rate / Da."""
    from pypanadapter_amd import Channelizer, Demodulator, Tap, chan_design, demod_design
    fs, M, Da = 64e3, 16, 2
    x = tp.noise_and_tones(16 * 8 * 40 + 5, 5)
    bank = Channelizer(fs, M)
    try:
        audio = Demodulator.for_channelizer(bank, "ssb", audio_decim=Da, bfo_hz=700.0)
        assert audio.rate == fs / 8 / Da and audio.group_delay == 8.0 and audio.streams == M
        used = audio.mode("ssb", bfo_hz=-700.0, first=3, count=2)
        word = round(-700.0 / (fs / 8) * 2 ** 32)
        assert used == word * (fs / 8) / 2 ** 32
        y = bank.push(x)
        a = np.concatenate([audio.push(y[:100]), audio.push(y[100:])])
        assert audio.steps_seen == len(y) and a.shape == (dr.steps(0, len(y), Da), M)
        g = demod_design(8 * Da + 1, 0.4 / Da).astype(np.float32)
        words = np.full(M, round(700.0 / (fs / 8) * 2 ** 32))
        words[3:5] = word
        _under(a, dr.ref_push(y, 0, dr.SSB, words, g, Da), dr.gate(g, dr.SSB, np.abs(y).max()), "Demodulator.for_channelizer")
        audio.close()
        with pytest.raises(ValueError, match="demod is off"):
            bank._plan.demod_state()
    finally:
        bank.close()
    taps = Tap(fs, max_taps=2, max_len=257)
    try:
        taps.open(1, 5e3, decim=16)
        audio = Demodulator.for_tap(taps, "power", audio_decim=4)
        assert audio.rate == fs / 16 / 4 and audio.streams == 1
        y = taps.push(x)[1]
        a = audio.push(y)
        g = demod_design(33, 0.1).astype(np.float32)
        _under(a, dr.ref_push(y.reshape(-1, 1), 0, dr.POWER, 0, g, 4), dr.gate(g, dr.POWER, np.abs(y).max()), "Demodulator.for_tap")
    finally:
        taps.close()


# ---------------------------------------------------------------- 10. off means off
def test_off_means_off():
    from pypanadapter_amd import ZoomFFT, synth
    x = np.stack([synth.make_iq(65536, 2.4e6, 3 + f, n_fft=1024, zoom=8, n_win=128) for f in range(16)])
    y = dr.noise_and_tones(500, 4, 3)
    with ZoomFFT(1024, 8, 2.4e6, n_win=128) as plan:
        plan.set_timing(True)
        rows = plan.rows(x)
        names = plan.launch_names()
        assert names and not [n for n in names if "demod" in n]
        for call in (plan.demod_state, plan.demod_shape, lambda: plan.demod_steps(5), lambda: plan.demod_push(y),
                     lambda: plan.demod_mode("fm"), lambda: plan.demod_mode(0, first=0, count=1), plan.demod_info,
                     plan.demod_reset, lambda: plan.demod_push_device(8, 1, 1, 1, 8)):
            with pytest.raises(ValueError, match="demod is off"):
                call()
        plan.set_demod(4, decim=2)                     # on: a process call is still the plan's alone
        assert plan.demod_shape() == (4, 17, 2)
        assert np.array_equal(plan.rows(x), rows) and plan.launch_names() == names
        a = plan.demod_push(y)
        assert plan.launch_names() == ["demod_push"] and len(plan.timings()) == 1 and a.shape == (250, 4)
        plan.set_demod(0)                              # off again, everything freed
        with pytest.raises(ValueError, match="demod is off"):
            plan.demod_shape()
        assert np.array_equal(plan.rows(x), rows) and plan.launch_names() == names
        plan.set_demod(0)


# ---------------------------------------------------------------- 11. calls and errors
def test_calls_and_errors():
    from pypanadapter_amd import ZoomFFT, _lib
    with ZoomFFT(32, 1, 1.0) as plan:
        g = np.ones(1024, np.float32)
        p = g.ctypes.data_as(ctypes.c_void_p)
        for K, Ta, Da in [(-1, 8, 1), (1025, 8, 1), (4, 0, 1), (4, -1, 1), (4, 1025, 1), (4, 8, 0), (4, 8, -1), (4, 8, 65)]:
            assert plan.lib.zfft_plan_demod(plan._plan, K, Ta, Da, p) == _lib.ZFFT_EINVAL, (K, Ta, Da)
        assert b"demod" in plan.lib.zfft_last_error()
        assert plan.lib.zfft_plan_demod(plan._plan, 4, 8, 2, None) == _lib.ZFFT_EINVAL    # without taps: 0 or 8 decim + 1
        with pytest.raises(ValueError, match="demod is off"):
            plan.demod_state()                          # a refused call enables nothing
        assert plan.lib.zfft_plan_demod(plan._plan, 4, 17, 2, None) == 0 and plan.demod_shape() == (4, 17, 2)
        plan.set_demod(3, taps=g[:8], decim=3)
        assert plan.demod_shape() == (3, 8, 3) and plan.demod_state() == 0
        for bad in [(-1, 1), (3, 1), (0, 0), (0, 4), (2, 2)]:
            with pytest.raises(ValueError, match="demod_mode"):
                plan.demod_mode("am", first=bad[0], count=bad[1])
        for m in (-1, 4):
            with pytest.raises(ValueError, match="demod_mode"):
                plan.demod_mode(m)
        assert plan.lib.zfft_demod_mode(plan._plan, 0, 1, 2, 2 ** 31) == _lib.ZFFT_EINVAL
        assert plan.lib.zfft_demod_mode(plan._plan, 0, 1, 2, -2 ** 31) == 0
        assert plan.demod_mode("ssb", bfo_hz=0.25) == 0.25 and plan.demod_mode("ssb", bfo_hz=0.75) == -0.25
        for n in (-1, 2 ** 31):
            with pytest.raises(ValueError):
                plan.demod_steps(n)
            with pytest.raises(ValueError):
                plan.demod_push_device(8, n, 3, 1, 8)
        for ss, ts in [(0, 1), (3, 0), (-3, 1), (3, -1), (2 ** 31 + 1, 1), (3, 2 ** 31 + 1)]:
            with pytest.raises(ValueError, match="stride"):
                plan.demod_push_device(8, 5, ss, ts, 8)
        with pytest.raises(ValueError, match="null"):
            plan.demod_push_device(0, 5, 3, 1, 8)
        with pytest.raises(ValueError, match="null"):
            plan.demod_push_device(8, 5, 3, 1, 0)
        with pytest.raises(ValueError, match="misaligned"):
            plan.demod_push_device(12, 5, 3, 1, 8)
        plan.demod_push_device(0, 0, 0, 0, 0)           # steps = 0: OK, nothing happens
        z = lambda n: np.zeros((n, 3), np.complex64)
        assert plan.demod_steps(0) == 0 and plan.demod_push(z(0)).shape == (0, 3)
        assert plan.demod_push(z(2)).shape == (1, 3) and plan.demod_state() == 2
        assert plan.demod_push(z(1)).shape == (0, 3) and plan.demod_state() == 3       # no output in it
        assert plan.demod_push(z(1)).shape == (1, 3)
        with pytest.raises(ValueError):
            plan.demod_push(np.zeros((2, 4), np.complex64))
        with pytest.raises(ValueError):
            plan.demod_push(np.zeros(6, np.complex64))  # 1-D: one stream only
        for n0 in (-1, 2 ** 62 + 1):
            with pytest.raises(ValueError):
                plan.demod_reset(n0)
        plan.demod_reset(2 ** 62 - 3)
        with pytest.raises(ValueError, match="2\\^62"):
            plan.demod_push(z(10))
        assert plan.lib.zfft_plan_demod(plan._plan, 4, 8, 65, p) == _lib.ZFFT_EINVAL
        assert plan.demod_shape() == (3, 8, 3)          # a refused call changes nothing
        plan.set_demod(1, decim=1)                      # re-enabling: the count at 0; one stream takes 1-D
        assert plan.demod_shape() == (1, 9, 1) and plan.demod_state() == 0
        assert plan.demod_info() == {"group_delay": 4.0, "rate_ratio": 1.0}
        assert plan.demod_push(np.ones(5, np.complex64)).shape == (5, 1)
        plan.demod_push_device(8, 0, 1, 0, 0)
