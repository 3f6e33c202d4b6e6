"""GPU checks of the channeliser (zfft_plan_chan; csrc/chan_kernels.hip) against tests/chan_ref.py,
the rule of include/zfft.h in numpy float64.  The error gate is derived, not measured:
|y - y_ref| <= (P + 5 log2 M + 2) 2^-24 sum|h| max|x| (chan_ref.gate); the impulse test, where a
window holds one non-zero sample, uses max|h| A for sum|h| max|x| (chan_ref.impulse_gate).  Every
comparison prints its worst ratio to the gate before it asserts.

Figures of the first run on an MI355X (worst |y - ref| / gate per test) are in
profiles/chan/README.md."""
import ctypes

import numpy as np
import pytest

import chan_ref as cr
import stall
import tap_ref as tp

pytestmark = pytest.mark.gpu
IDS = [f"M{M}-P{P}-D{D}" for M, P, D in cr.CASES]


@pytest.fixture(scope="module", autouse=True)
def _gpu(zfft_lib):
    from pypanadapter_amd import device_count
    assert device_count() >= 1, "GPU tests need a HIP device"


def _proto(M, P):
    """The default prototype where P = 8, caller-supplied solid taps elsewhere; float32."""
    from pypanadapter_amd import chan_design
    return chan_design(M, P, 8.0).astype(np.float32) if P == 8 else tp.solid_taps(M * P, 100 + M + P)


def _plan(M, P, D, h=None, in_dtype="complex64", fs=1.0, default=False):
    """A plan with the bank on; default: the library designs the prototype (taps=None)."""
    from pypanadapter_amd import ZoomFFT
    plan = ZoomFFT(32, 1, fs, in_dtype=in_dtype)
    plan.set_channels(M, P, M // D, taps=None if default else (_proto(M, P) if h is None else h))
    return plan


def _under(got, ref, bound, what):
    err = float(np.abs(got.astype(np.complex128) - ref).max()) if ref.size else 0.0
    print(f"{what}: max|y - ref| = {err:.3e} = {err / bound:.4f} of the gate {bound:.3e}")
    assert got.shape == ref.shape and err <= bound, (what, err, bound)
    return err / bound


def _form(plan, n0, n):
    from test_chan_host import chan_form
    M, P, D, _, K = plan.chan_shape()
    return chan_form(plan.lib, n0, n, M, P, D, K)


def _signed_word(c, M):
    return (c * 2 ** 32 // M + 2 ** 31) % 2 ** 32 - 2 ** 31


# ---------------------------------------------------------------- 1. impulses
@pytest.mark.parametrize("M,P,D", cr.CASES, ids=IDS)
def test_impulses_at_the_residues_and_across_a_span_boundary(M, P, D):
    A = 0.75
    T = M * P
    h = _proto(M, P)
    span = 1024 // M * D                              # a push this short runs at 1024 points a span
    gap = -(-(T + D) // D) * D + D                    # no two impulses share a step's window
    residues = list(range(M)) if M <= 64 else [0, 1, D - 1, D, M - 1]
    pos = [span - 1]                                  # the last sample of a span ...
    pos.append(span * -(-(pos[0] + gap) // span))     # ... and the first of another
    for r in residues:
        p = pos[-1] + gap
        pos.append(p + (r - p) % M)
    n = pos[-1] + gap + 3
    n += n % span == 0                                # a ragged tail
    assert sorted({p % M for p in pos[2:]}) == sorted(residues) and min(np.diff(pos)) >= gap
    x = np.zeros(n, np.complex64)
    x[pos] = A * np.exp(2j * np.pi * 0.37 * np.arange(len(pos)))
    with _plan(M, P, D, h, default=(P == 8)) as plan:
        f = _form(plan, 0, n)
        assert f["span"] == span and f["nspans"] >= 3 and n % span and pos[0] % span == span - 1 and pos[1] % span == 0
        assert plan.chan_steps(n) == cr.steps(0, n, D)
        y = plan.chan_push(x)
    ref = cr.ref_push(x, 0, M, D, h)
    _under(y, ref, cr.impulse_gate(h, M, P, A), f"impulses M={M} P={P} D={D}")
    empty = ~ref.any(axis=1)                          # the steps whose window holds no impulse
    assert empty.any() and not empty.all()
    assert not y[empty].any()                         # exactly 0
    assert y[~empty].all() and ref[~empty].all()      # every channel sees every impulse


# ---------------------------------------------------------------- 2. noise plus tones
@pytest.mark.parametrize("M,P,D", cr.CASES, ids=IDS)
def test_noise_and_tones_under_the_derived_gate(M, P, D):
    T = M * P
    span = 1024 // M * D
    n = 2 * span + 301 + T                            # at least two spans and a ragged tail
    x = tp.noise_and_tones(n, 7 + M)
    h = _proto(M, P)
    with _plan(M, P, D, h, default=(P == 8)) as plan:
        f = _form(plan, 0, n)
        assert f["span"] == span and f["nspans"] >= 3 and n % span
        assert plan.chan_shape() == (M, P, D, 0, M)
        assert plan.chan_info() == {"group_delay": (T - 1) / 2, "rate_ratio": 1.0 / D}
        y = plan.chan_push(x)
        assert plan.chan_state() == n
    ms = cr.step_indices(0, n, D)
    gate = cr.gate(h, M, P, np.abs(x).max())
    _under(y, cr.ref_chan(x, 0, M, D, h, ms), gate, f"noise M={M} P={P} D={D}")
    for c in (0, 1, M // 2, M - 1):                   # the rule's other form: a tap at c 2^32 / M
        want = tp.ref_tap(x, 0, _signed_word(c, M), D, h, np.array(ms, dtype=np.int64))
        _under(y[:, c], want, gate, f"  channel {c} against the tap reference")


# ---------------------------------------------------------------- 3. against the tap kernel
def test_against_the_tap_kernel_on_the_device():
    M, P, D = 64, 8, 32
    T = M * P
    n = 2 * 512 + 301 + T
    x = tp.noise_and_tones(n, 31)
    h = _proto(M, P)
    chans = (1, M // 2, M - 1)
    with _plan(M, P, D, h) as plan:
        plan.set_taps(4, T)
        for s, c in enumerate(chans):
            plan.tap_open(s, c / M, D, taps=h)        # (fs = 1)
            assert plan.tap_info(s)["freq_word"] == _signed_word(c, M)
        taps = plan.tap_push(x)
        y = plan.chan_push(x)
        assert plan.tap_state() == plan.chan_state() == n
    bound = cr.gate(h, M, P, np.abs(x).max()) + tp.gate(h, np.abs(x).max())
    for s, c in enumerate(chans):
        _under(y[:, c], taps[s].astype(np.complex128), bound, f"channel {c} against its tap on the device")


# ---------------------------------------------------------------- 4. split invariance
@pytest.mark.parametrize("M,P,D", cr.CASES, ids=IDS)
def test_outputs_do_not_depend_on_the_cut_bit_for_bit(M, P, D):
    T = M * P
    cut = [1, 1, 7, D - 1, T - 2, T - 1, T, 1023]
    n = sum(cut) + 1500 + D
    cut.append(n - sum(cut))
    x = tp.noise_and_tones(n, 21 + M)
    h = _proto(M, P)
    with _plan(M, P, D, h) as plan:
        whole = plan.chan_push(x)
        assert plan.chan_state() == n
    with _plan(M, P, D, h) as plan:
        parts, at = [], 0
        for c in cut:
            want = plan.chan_steps(c)
            assert want == cr.steps(at, c, D)
            parts.append(plan.chan_push(x[at:at + c]))
            assert parts[-1].shape == (want, M)
            at += c
        assert plan.chan_state() == n
    parts = np.concatenate(parts)
    assert parts.shape == whole.shape == (cr.steps(0, n, D), M)
    assert parts.tobytes() == whole.tobytes()


# ---------------------------------------------------------------- 5. counts past 2^32
@pytest.mark.parametrize("n0", [2 ** 32 - 100, 2 ** 40 + 3])
def test_a_count_past_2_to_the_32(n0):
    x = tp.noise_and_tones(5000, 51)
    for M, P, D in [(64, 8, 32), (16, 4, 16), (128, 4, 64)]:
        assert n0 % D                                  # the first step is not the first sample
        h = _proto(M, P)
        with _plan(M, P, D, h) as plan:
            plan.chan_reset(n0)
            assert plan.chan_state() == n0 and plan.chan_steps(2777) == cr.steps(n0, 2777, D)
            a = plan.chan_push(x[:2777])
            b = plan.chan_push(x[2777:])
            assert plan.chan_state() == n0 + 5000
        _under(np.concatenate([a, b]), cr.ref_push(x, n0, M, D, h), cr.gate(h, M, P, np.abs(x).max()),
               f"n0={n0} M={M} D={D}")


# ---------------------------------------------------------------- 6. the other input formats
@pytest.mark.parametrize("in_dtype", ["complex32", "cu8", "f32"])
def test_each_other_input_format(in_dtype):
    M, P, D, n = 16, 4, 8, 2 * 512 + 301
    z = tp.noise_and_tones(n, 61)
    if in_dtype == "complex32":
        raw = np.stack([z.real, z.imag], axis=1).astype(np.float16).reshape(-1)
    elif in_dtype == "cu8":
        raw = np.clip(np.round(np.stack([z.real, z.imag], axis=1) / 1.5 * 127.5 + 127.5), 0, 255).astype(np.uint8).reshape(-1)
    else:
        raw = z.real.astype(np.float32)
    x = tp.loader(raw, in_dtype)                     # the float32 values the loader defines
    h = _proto(M, P)
    two = in_dtype in ("complex32", "cu8")
    with _plan(M, P, D, h, in_dtype=in_dtype) as plan:
        a = plan.chan_push(raw[:2 * 333] if two else raw[:333])
        b = plan.chan_push(raw[2 * 333:] if two else raw[333:])
    _under(np.concatenate([a, b]), cr.ref_push(x, 0, M, D, h), cr.gate(h, M, P, np.abs(x).max()), in_dtype)


def test_flip_input_is_unsupported():
    from pypanadapter_amd import ZoomFFT
    with ZoomFFT(32, 1, 1.0, flip=True) as plan:
        with pytest.raises(NotImplementedError, match="flip_input"):
            plan.set_channels(16, 4)
        with pytest.raises(ValueError, match="channels are off"):
            plan.chan_state()


# ---------------------------------------------------------------- 7. selection
def test_select_keeps_columns_bit_for_bit_and_writes_nothing_else():
    import torch
    M, P, D = 64, 8, 32
    n = 2 * 512 + 301
    x = tp.noise_and_tones(n, 71)
    steps = cr.steps(0, n, D)
    with _plan(M, P, D) as plan:
        full = plan.chan_push(x)
        for c0, k in [(5, 7), (60, 9), (M // 2, M), (M - 1, 1), (0, 1), (17, M)]:
            plan.chan_reset(0)
            plan.chan_select(c0, k)
            assert plan.chan_shape() == (M, P, D, c0, k)
            cols = (c0 + np.arange(k)) % M
            got = plan.chan_push(x)
            assert got.shape == (steps, k) and got.tobytes() == np.ascontiguousarray(full[:, cols]).tobytes(), (c0, k)
            f = plan.chan_freqs()
            assert np.array_equal(f, np.where(cols >= M // 2, cols - M, cols) / M)
        plan.chan_select(M // 2, M)                   # ascending frequency: the fftshift
        plan.chan_reset(0)
        assert np.array_equal(plan.chan_push(x), np.fft.fftshift(full, axes=1))
        assert np.all(np.diff(plan.chan_freqs()) > 0)
        # a device push: nothing beyond steps x K is written
        k, guard = 9, 64
        plan.chan_select(60, k)
        plan.chan_reset(0)
        d_x = torch.from_numpy(x.view(np.float32).reshape(-1, 2).copy()).to("cuda")
        d_y = stall.sentinel((steps * k + guard, 2))
        plan.chan_push_device(d_x.data_ptr(), n, d_y.data_ptr())
        torch.cuda.synchronize()
        out = d_y.cpu().numpy()
        assert (out[steps * k:] == stall.SENTINEL).all()
        got = np.ascontiguousarray(out[:steps * k]).view(np.complex64).reshape(steps, k)
        assert got.tobytes() == np.ascontiguousarray(full[:, (60 + np.arange(k)) % M]).tobytes()


# ---------------------------------------------------------------- 8. physical sanity
def test_a_tone_comes_out_of_its_channel_at_the_prototypes_gain():
    """From the prototype alone: a tone at the centre of channel c0 leaves channel c at
    amp |H((c0 - c) / M)|, H the prototype's response -- |H(0)| in its own channel, and in every
    non-adjacent one no more than max|H| over that channel's range of offsets; a tone on the edge
    between two channels leaves both at the same magnitude."""
    M, P, D, amp = 64, 8, 32, 0.5
    T = M * P
    h = _proto(M, P)
    h64 = h.astype(np.float64)
    H = lambda nu: np.abs(np.exp(-2j * np.pi * np.outer(np.atleast_1d(nu), np.arange(T))) @ h64)
    n = 6 * T
    t = np.arange(n)
    skip = T // D + 1                                 # past the filter's start
    gate = cr.gate(h, M, P, amp)
    with _plan(M, P, D, h) as plan:
        c0 = 11
        x = (amp * np.exp(2j * np.pi * (c0 / M) * t)).astype(np.complex64)
        y = np.abs(plan.chan_push(x)[skip:].astype(np.complex128))
        ref = np.abs(cr.ref_push(x, 0, M, D, h)[skip:])
        print(f"centre tone: own channel {y[:, c0].max():.6f} (amp |H(0)| = {amp * H(0.0)[0]:.6f}); "
              f"worst non-adjacent channel {np.delete(y, [c0 - 1, c0, c0 + 1], axis=1).max():.3e}")
        # the input is rounded to float32 once: 2^-24 amp sum|h| on top of the gate
        slack = gate + 2.0 ** -24 * amp * np.abs(h64).sum()
        assert np.abs(y[:, c0] - amp * H(0.0)[0]).max() <= slack and np.abs(ref[:, c0] - amp * H(0.0)[0]).max() <= slack
        for c in range(M):
            if min((c - c0) % M, (c0 - c) % M) <= 1:
                continue
            nu = (c0 - c) / M + np.linspace(-0.5 / M, 0.5 / M, 33)
            assert y[:, c].max() <= amp * H(nu).max() + slack, c
        c1 = 40
        plan.chan_reset(0)
        x = (amp * np.exp(2j * np.pi * ((c1 + 0.5) / M) * t)).astype(np.complex64)
        y = np.abs(plan.chan_push(x)[skip:].astype(np.complex128))
        want = amp * H(0.5 / M)[0]
        print(f"edge tone: channels {c1}, {c1 + 1} at {y[:, c1].max():.6f}, {y[:, c1 + 1].max():.6f} (amp |H(1/2M)| = {want:.6f})")
        assert np.abs(y[:, c1] - y[:, c1 + 1]).max() <= 2 * slack
        assert np.abs(y[:, c1] - want).max() <= slack and abs(H(0.5 / M)[0] - H(-0.5 / M)[0]) <= 1e-12


# ---------------------------------------------------------------- 9. ordering
def test_a_device_push_behind_a_stalled_stream():
    """process_device on A and, right after it, a bank push of the same buffer on B and another on C,
    enqueued while a bounded spin kernel holds A (tests/stall.py): nothing runs ahead of the plan's
    earlier work, no enqueue waits on the host, and both results are right."""
    import torch
    from pypanadapter_amd import ZoomFFT
    streams = stall.streams()
    F, L, N, M, P, D = 4, 4096, 1024, 16, 4, 8
    x = tp.noise_and_tones(F * L, 71)
    h = _proto(M, P)
    half = F * L // 2

    def bufs():
        return {"x": torch.from_numpy(x.view(np.float32).reshape(F, L, 2).copy()).to("cuda"),
                "rows": stall.sentinel((F, N)), "y": stall.sentinel((F * L // D * M, 2))}

    def seq(plan, run, b):
        run.call("process", plan.process_device, b["x"].data_ptr(), L, F, b["rows"].data_ptr(), on=streams[0])
        run.call("chan_push0", plan.chan_push_device, b["x"].data_ptr(), half, b["y"].data_ptr(), on=streams[1])
        run.call("chan_push1", plan.chan_push_device, b["x"].data_ptr() + 8 * half, F * L - half,
                 b["y"].data_ptr() + 8 * (half // D) * M, on=streams[2])

    def make():
        plan = ZoomFFT(N, 1, 1.0)
        plan.set_channels(M, P, M // D, taps=h)
        seq(plan, stall.Run(plan, streams, held=False), bufs())   # the workspaces have their size
        torch.cuda.synchronize()
        plan.chan_reset(0)
        torch.cuda.synchronize()
        return plan, bufs()

    def sequence(plan, run, b):
        seq(plan, run, b)
        run.check_order()
        return {"rows": b["rows"], "y": b["y"]}

    held, stepped, run = stall.enqueue_twice("chan[push]", make, sequence, streams)
    assert run.final_held and run.quiesce_delta == 0             # no host wait in any enqueue
    stall.same_bytes(held, stepped, "held")
    assert not (held["rows"] == stall.SENTINEL).any()
    y = np.ascontiguousarray(held["y"]).view(np.complex64).reshape(-1, M)
    _under(y, cr.ref_push(x, 0, M, D, h), cr.gate(h, M, P, np.abs(x).max()), "device pushes")
    with ZoomFFT(N, 1, 1.0) as plan:
        np.testing.assert_allclose(plan.rows(x.reshape(F, L)), held["rows"], rtol=0, atol=1e-3)


# ---------------------------------------------------------------- 10. off means off
def test_off_means_off():
    from pypanadapter_amd import ZoomFFT, synth
    x = np.stack([synth.make_iq(65536, 2.4e6, 3 + f, n_fft=1024, zoom=8, n_win=128) for f in range(16)])
    with ZoomFFT(1024, 8, 2.4e6, n_win=128) as plan:
        plan.set_timing(True)
        rows = plan.rows(x)
        names = plan.launch_names()
        assert names and not [n for n in names if "chan" in n]
        for call in (plan.chan_state, plan.chan_shape, lambda: plan.chan_steps(5), lambda: plan.chan_push(x[0]),
                     lambda: plan.chan_select(0, 1), plan.chan_info, plan.chan_reset, plan.chan_freqs,
                     lambda: plan.chan_push_device(8, 1, 8)):
            with pytest.raises(ValueError, match="channels are off"):
                call()
        plan.set_channels(64)                         # on: a process call is still the plan's alone
        assert plan.chan_shape() == (64, 8, 32, 0, 64)
        assert np.array_equal(plan.rows(x), rows) and plan.launch_names() == names
        y = plan.chan_push(x[0])
        assert plan.launch_names() == ["chan_push"] and len(plan.timings()) == 1 and y.shape == (65536 // 32, 64)
        plan.set_channels(0)                          # off again, everything freed
        with pytest.raises(ValueError, match="channels are off"):
            plan.chan_shape()
        assert np.array_equal(plan.rows(x), rows) and plan.launch_names() == names
        plan.set_channels(0)


# ---------------------------------------------------------------- 11. calls and errors
def test_calls_and_errors():
    from pypanadapter_amd import ZoomFFT, _lib
    with ZoomFFT(32, 1, 1.0) as plan:
        h = np.ones(64, np.float32)
        p = h.ctypes.data_as(ctypes.c_void_p)
        for M, P, D in [(4, 8, 4), (12, 4, 12), (2048, 1, 2048), (-8, 1, 8), (8, 0, 8), (8, -1, 8), (8, 257, 8),
                        (1024, 3, 512), (8, 8, 2), (8, 8, 16), (8, 8, 0), (8, 8, 3)]:
            assert plan.lib.zfft_plan_chan(plan._plan, M, P, D, p) == _lib.ZFFT_EINVAL, (M, P, D)
        assert b"chan" in plan.lib.zfft_last_error()
        with pytest.raises(ValueError, match="channels are off"):
            plan.chan_state()                          # a refused call enables nothing
        with pytest.raises(ValueError):
            plan.set_channels(8, 8, oversample=3)
        with pytest.raises(ValueError):
            plan.set_channels(8, 8, taps=np.ones(63, np.float32))
        plan.set_channels(8, 8, 2, taps=h)
        assert plan.chan_shape() == (8, 8, 4, 0, 8) and plan.chan_state() == 0
        for bad in [(-1, 1), (8, 1), (0, 0), (0, 9), (3, -1)]:
            with pytest.raises(ValueError, match="chan_select"):
                plan.chan_select(*bad)
        assert plan.chan_shape()[3:] == (0, 8)
        plan.chan_select(6, 5)
        for n in (-1, 2 ** 31):
            with pytest.raises(ValueError):
                plan.chan_steps(n)
            with pytest.raises(ValueError):
                plan.chan_push_device(8, n, 8)
        with pytest.raises(ValueError, match="null"):
            plan.chan_push_device(0, 5, 8)
        with pytest.raises(ValueError, match="null"):
            plan.chan_push_device(8, 5, 0)
        plan.chan_push_device(0, 0, 0)                 # n_samples = 0: OK, nothing happens
        assert plan.chan_steps(0) == 0 and plan.chan_push(np.zeros(0, np.complex64)).shape == (0, 5)
        assert plan.chan_push(np.zeros(3, np.complex64)).shape == (1, 5) and plan.chan_state() == 3
        assert plan.chan_push(np.zeros(1, np.complex64)).shape == (0, 5) and plan.chan_state() == 4   # no step in it
        assert plan.chan_push(np.zeros(1, np.complex64)).shape == (1, 5)
        with pytest.raises(ValueError):
            plan.chan_push(np.zeros((2, 8), np.complex64))
        for n0 in (-1, 2 ** 62 + 1):
            with pytest.raises(ValueError):
                plan.chan_reset(n0)
        plan.chan_reset(2 ** 62 - 3)
        assert plan.chan_shape()[3:] == (6, 5)         # a reset keeps the selection
        with pytest.raises(ValueError, match="2\\^62"):
            plan.chan_push(np.zeros(10, np.complex64))
        assert plan.lib.zfft_plan_chan(plan._plan, 8, 8, 16, p) == _lib.ZFFT_EINVAL
        assert plan.chan_shape() == (8, 8, 4, 6, 5)    # a refused call changes nothing
        plan.set_channels(16, 4, 1, taps=h)            # re-enabling: the count at 0, all channels selected
        assert plan.chan_shape() == (16, 4, 16, 0, 16) and plan.chan_state() == 0
        assert plan.chan_info() == {"group_delay": 31.5, "rate_ratio": 1.0 / 16}
        assert np.array_equal(plan.chan_freqs(), np.where(np.arange(16) >= 8, np.arange(16) - 16, np.arange(16)) / 16)


# ---------------------------------------------------------------- 12. the largest span
def test_the_largest_span_on_a_long_push():
    """4096-point spans (64 steps of 64 channels; a push of at least 512 of them): the steps around
    the first span boundaries, some in the middle and the ragged end against the reference."""
    M, P, D = 64, 8, 32
    span = 4096 // M * D
    n = span * 600 + 77
    x = tp.noise_and_tones(n, 11)
    h = _proto(M, P)
    with _plan(M, P, D, default=True) as plan:
        f = _form(plan, 0, n)
        assert f["points"] == 4096 and f["span"] == span == 2048 and f["nspans"] == 601 and f["grid"] == 601
        y = plan.chan_push(x)
    steps = cr.steps(0, n, D)
    assert y.shape == (steps, M)
    per = span // D
    ms = np.unique(np.concatenate([np.arange(0, 3 * per + 4), np.arange(317 * per - 20, 317 * per + 20),
                                   np.arange(steps - 40, steps)]))
    _under(y[ms], cr.ref_chan(x, 0, M, D, h, [int(m) for m in ms]), cr.gate(h, M, P, np.abs(x).max()), "span 2048")


def test_more_spans_than_workgroups():
    """A push of more than 1024 spans: the workgroups walk the spans round-robin."""
    M, P, D = 1024, 2, 512
    span = 2048 // M * D                              # LDS holds 2048 points here: two steps a span
    n = span * 1300 + 513
    x = tp.noise_and_tones(n, 13)
    h = _proto(M, P)
    with _plan(M, P, D, h) as plan:
        f = _form(plan, 0, n)
        assert f["points"] == 2048 and f["span"] == span == 1024 and f["nspans"] == 1301 and f["grid"] == 1024
        y = plan.chan_push(x)
    steps = cr.steps(0, n, D)
    ms = np.unique(np.concatenate([np.arange(0, 6), np.arange(2 * 1023 - 3, 2 * 1024 + 5), np.arange(steps - 6, steps)]))
    _under(y[ms], cr.ref_chan(x, 0, M, D, h, [int(m) for m in ms]), cr.gate(h, M, P, np.abs(x).max()), "1301 spans on 1024 workgroups")


# ---------------------------------------------------------------- 13. the loop closed
def test_a_track_maps_to_its_channel():
    """Two tones 1 kHz apart beside a full-scale carrier: the detector and the tracker find the pair,
    Channelizer.channel_for maps the track's extent to the channel that holds it, and that channel's
    stream shows the two tones where they lie from the channel's centre, at the prototype's gain."""
    from pypanadapter_amd import Channelizer, Detector, chan_design, psd_lines, synth
    fs, N, rows, M = 512e3, 1024, 300, 32
    f_pair, f_car, amp = 60e3, -150e3, 0.1
    n = (rows + 1) * N // 2
    x = synth.tone_pair(n, fs, 81, f_centre=f_pair, spacing=1e3, amp=amp, carrier=(f_car, 1.0), noise=2e-3)
    lines = psd_lines(x, fs, N, 1, 1, window="blackmanharris")
    det = Detector(threshold_db=40.0, min_width=2, track=(1, 1, 50))
    try:
        det.update(lines)
        op = det.open_tracks()
        ext = det.track_extent(op, fs, N, 1, line_period=0.5 * N / fs)
    finally:
        det.close()
    assert len(op) == 2
    i = int(np.argmin(np.abs(ext["f_peak"] - f_pair)))
    bank = Channelizer(fs, M)
    try:
        col = bank.channel_for(ext, i)
        f_c = bank.freqs[col]
        assert f_c == 64e3 and abs(f_c - f_pair) <= 0.5 * fs / M          # the channel that holds the pair
        assert col == bank.channel_of(f_pair) == M // 2 + 4 and np.all(np.diff(bank.freqs) > 0)
        assert bank.channel_of(f_car) == M // 2 + int(round(f_car / (fs / M)))
        assert bank.rate == fs / 16 and bank.group_delay == (M * 8 - 1) / 2
        y = np.concatenate([bank.push(x[:n // 3]), bank.push(x[n // 3:])])
        assert bank.samples_seen == n and y.shape == (cr.steps(0, n, 16), M)
    finally:
        bank.close()
    D, T = 16, M * 8
    h = chan_design(M, 8).astype(np.float32)
    ref = cr.ref_push(x, 0, M, D, h)
    _under(y, np.fft.fftshift(ref, axes=1), cr.gate(h, M, 8, np.abs(x).max()), "Channelizer")
    s = y[:, col]
    skip = T // D + 1
    w = np.blackman(s.size - skip) * np.kaiser(s.size - skip, 20.0)
    w /= w.sum()
    m = np.arange(skip, s.size)                       # step m is sample m D: the phase of a tone at f is 2 pi f m D / fs
    H = lambda f: abs(np.sum(h.astype(np.float64) * np.exp(-2j * np.pi * f / fs * np.arange(T))))
    for side in (-500.0, 500.0):
        f = f_pair + side - f_c                       # where the tone lies from the channel's centre
        got = abs(np.sum(w * s[skip:].astype(np.complex128) * np.exp(-2j * np.pi * f / (fs / D) * m)))
        print(f"tone at {f:+.1f} Hz from the channel's centre: {got:.5f} (amp {amp} x |H| {H(f):.5f})")
        assert abs(got - amp * H(f)) <= 1e-3 * amp
