"""GPU checks of the channel taps (zfft_plan_taps; csrc/tap_kernels.hip) against tests/tap_ref.py,
the rule of include/zfft.h in numpy float64.  The error gate is derived, not measured:
|y - y_ref| <= (T + 32) 2^-24 sum|h| max|x| (tap_ref.gate); the impulse test, where every output
has one non-zero product, uses 32 2^-24 max|h| |A|.  Every comparison prints its worst ratio to
the gate before it asserts."""
import ctypes

import numpy as np
import pytest

import stall
import tap_ref as tp

pytestmark = pytest.mark.gpu
FW = tp.freq_word(0.0731, 1.0)   # an arbitrary non-zero word


@pytest.fixture(scope="module", autouse=True)
def _gpu(zfft_lib):
    from pypanadapter_amd import device_count
    assert device_count() >= 1, "GPU tests need a HIP device"


def _plan(max_taps=4, max_len=2048, in_dtype="complex64", fs=1.0):
    from pypanadapter_amd import ZoomFFT
    plan = ZoomFFT(32, 1, fs, in_dtype=in_dtype)
    plan.set_taps(max_taps, max_len)
    return plan


def _design(D, T):
    from pypanadapter_amd import tap_design
    return tap_design(T, 0.4 / D, 8.0).astype(np.float32)


def _under(got, ref, bound, what):
    err = float(np.abs(got.astype(np.complex128) - ref).max()) if len(ref) else 0.0
    print(f"{what}: max|y - ref| = {err:.3e} = {err / bound:.4f} of the gate {bound:.3e}")
    assert got.shape == ref.shape and err <= bound, (what, err, bound)
    return err / bound


def _form_span(plan, n0, n, taps):
    from test_tap_host import tap_form
    return tap_form(plan.lib, n0, n, plan.tap_shape()[1], taps)[0]["span"]


# ---------------------------------------------------------------- 1. impulse
@pytest.mark.parametrize("D,T", tp.DT_TAPS)
def test_impulses_at_every_residue_and_across_a_span_boundary(D, T):
    A = 0.75
    h = tp.solid_taps(T, 100 + D)
    gap = -(-(T + D) // D) * D                       # no two responses share an output
    pos = [511, 512 * -(-(511 + gap) // 512)]        # the last sample of a span, the first of another
    for r in range(D):                               # then one impulse per residue mod D
        pos.append(pos[-1] + gap + 1)
    n = pos[-1] + gap
    assert len({p % D for p in pos[1:]}) == D
    x = np.zeros(n, np.complex64)
    x[pos] = A * np.exp(2j * np.pi * 0.37 * np.arange(len(pos)))
    with _plan() as plan:
        assert _form_span(plan, 0, n, [(FW, D, T, 0)]) == 512 and pos[0] % 512 == 511 and pos[1] % 512 == 0
        assert plan.tap_open(0, 0.0731, D, taps=h) == FW / 2.0 ** 32
        (y,) = plan.tap_push(x)
    ref = tp.ref_push(x, 0, FW, D, h)
    _under(y, ref, 32 * 2.0 ** -24 * float(np.abs(h).max()) * A, f"impulse D={D} T={T}")
    assert np.array_equal(y == 0, ref == 0)          # no tap dropped, none where there is no sample


# ---------------------------------------------------------------- 2. noise plus tones
@pytest.mark.parametrize("D,T", tp.DT_TAPS)
def test_noise_and_tones_under_the_derived_gate(D, T):
    n = 2 * 512 + 301 + (T if T > 1024 else 0)       # two spans and a ragged tail
    x = tp.noise_and_tones(n, 7 + D)
    h = _design(D, T)
    with _plan() as plan:
        assert _form_span(plan, 0, n, [(FW, D, T, 0)]) == 512
        if T == 8 * D + 1:
            plan.tap_open(0, 0.0731, D)              # the default design: T = 8 D + 1, cutoff 0.4 / D, beta 8
        else:
            plan.tap_open(0, 0.0731, D, taps=h)
        info = plan.tap_info(0)
        assert (info["n_taps"], info["decim"], info["freq_word"], info["group_delay"]) == (T, D, FW, (T - 1) / 2)
        (y,) = plan.tap_push(x)
    _under(y, tp.ref_push(x, 0, FW, D, h), tp.gate(h, np.abs(x).max()), f"noise D={D} T={T}")


def test_the_largest_span_on_a_long_push():
    """4096-sample spans (a push of at least 2^22 samples): the outputs around the first span
    boundaries, one in the middle and the ragged end against the reference."""
    D, T = 32, 257
    n = 4096 * 1024 + 77
    x = tp.noise_and_tones(n, 11)
    h = _design(D, T)
    with _plan() as plan:
        assert _form_span(plan, 0, n, [(FW, D, T, 0)]) == 4096
        plan.tap_open(0, 0.0731, D)
        (y,) = plan.tap_push(x)
    assert y.size == tp.count(0, 0, n, D)
    ms = np.unique(np.concatenate([np.arange(0, 400), np.arange(4096 * 517 // D - 150, 4096 * 517 // D + 150),
                                   np.arange(y.size - 300, y.size)]))
    _under(y[ms], tp.ref_tap(x, 0, FW, D, h, ms), tp.gate(h, np.abs(x).max()), "span 4096")


# ---------------------------------------------------------------- 3. split invariance
@pytest.mark.parametrize("D,T", tp.DT_TAPS)
def test_outputs_do_not_depend_on_the_cut_bit_for_bit(D, T):
    cut = [1, 1, 7, D - 1, max(T - 2, 0), T - 1, T, 1023]
    n = sum(cut) + 1500 + D
    cut.append(n - sum(cut))
    x = tp.noise_and_tones(n, 21 + D)
    h = tp.solid_taps(T, 5) if T < 100 else _design(D, T)
    with _plan() as plan:
        plan.tap_open(2, 0.0731, D, taps=h)
        (whole,) = plan.tap_push(x)
        assert plan.tap_state() == n
    with _plan() as plan:
        plan.tap_open(2, 0.0731, D, taps=h)
        parts, at = [], 0
        for c in cut:
            want = tp.count(at, 0, c, D)
            assert plan.tap_counts(c).tolist() == [0, 0, want, 0], (at, c)
            got = plan.tap_push(x[at:at + c])
            assert len(got) == 1 and got[0].size == want
            parts.append(got[0])
            at += c
            assert plan.tap_state() == at
    assert np.concatenate(parts).tobytes() == whole.tobytes()
    _under(whole, tp.ref_push(x, 0, FW, D, h), tp.gate(h, np.abs(x).max()), f"whole D={D} T={T}")


# ---------------------------------------------------------------- 4. several taps in one push
def test_four_taps_in_one_push_equal_each_alone_and_a_late_tap_sees_the_past():
    taps = [(0.0731, 8, tp.solid_taps(65, 1)), (-0.211, 3, tp.solid_taps(25, 2)), (0.4999, 32, _design(32, 257)),
            (0.0, 200, _design(200, 1601))]
    late = (0.013, 5, tp.solid_taps(41, 9))
    n1, n2 = 2 * 512 + 333, 1024 + 77
    x = tp.noise_and_tones(n1 + n2, 31)
    with _plan() as plan:
        for s, (f, D, h) in enumerate(taps):
            plan.tap_open(s, f, D, taps=h)
        first = plan.tap_push(x[:n1])
        plan.tap_close(1)
        plan.tap_open(1, late[0], late[1], taps=late[2])     # opened at n1, not a multiple of 5
        assert plan.tap_info(1)["n_open"] == n1 and plan.tap_counts(n2)[1] == tp.count(n1, n1, n2, 5)
        plan.tap_close(3)
        second = plan.tap_push(x[n1:])
        assert len(first) == 4 and len(second) == 3
    together = {0: (first[0], second[0]), 1: (first[1], None), 2: (first[2], second[2]), 3: (first[3], None)}
    for s, (f, D, h) in enumerate(taps):
        with _plan() as plan:
            plan.tap_open(s, f, D, taps=h)
            (a,) = plan.tap_push(x[:n1])
            (b,) = plan.tap_push(x[n1:])
        assert a.tobytes() == together[s][0].tobytes(), s
        if together[s][1] is not None:
            assert b.tobytes() == together[s][1].tobytes(), s
        fw = tp.freq_word(f, 1.0)
        _under(np.concatenate([a, b]), tp.ref_push(x, 0, fw, D, h), tp.gate(h, np.abs(x).max()), f"alone slot {s}")
    # the late tap: alone on a plan that saw the same past; its grid starts at the first m D >= n_open
    with _plan() as plan:
        assert plan.tap_push(x[:n1]) == []                   # no tap open: the carry is still kept
        plan.tap_open(0, late[0], late[1], taps=late[2])
        (alone,) = plan.tap_push(x[n1:])
    assert alone.tobytes() == second[1].tobytes()
    ms = tp.outputs(n1, n1, n2, late[1])
    assert ms[0] == -(-n1 // 5) and ms[0] * 5 > n1 and alone.size == ms.size
    ref = tp.ref_tap(x, 0, tp.freq_word(late[0], 1.0), late[1], late[2], ms)    # the true past, not zeros
    _under(alone, ref, tp.gate(late[2], np.abs(x).max()), "late tap")
    zero_past = tp.ref_tap(x[n1:], n1, tp.freq_word(late[0], 1.0), late[1], late[2], ms)
    assert np.abs(zero_past[:4] - ref[:4]).max() > 100 * tp.gate(late[2], np.abs(x).max())   # (the past matters here)


def test_short_pushes_compose_the_carry():
    """Pushes far shorter than max_len - 1, down to one sample, with the longest filter."""
    D, T = 7, 2048
    h = _design(D, T)
    x = tp.noise_and_tones(2600, 41)
    cut = [1, 1, 2, 3, 100, 1, 2047, 1, 300, 144]
    assert sum(cut) == x.size
    with _plan() as plan:
        plan.tap_open(0, 0.0731, D, taps=h)
        parts, at = [], 0
        for c in cut:
            parts += plan.tap_push(x[at:at + c])
            at += c
    y = np.concatenate(parts)
    _under(y, tp.ref_push(x, 0, FW, D, h), tp.gate(h, np.abs(x).max()), "short pushes")
    with _plan() as plan:
        plan.tap_open(0, 0.0731, D, taps=h)
        assert plan.tap_push(x)[0].tobytes() == y.tobytes()


# ---------------------------------------------------------------- 5. long streams without pushing them
@pytest.mark.parametrize("n0", [2 ** 32 - 100, 2 ** 40 + 3])
def test_a_count_past_the_phase_wrap(n0):
    x = tp.noise_and_tones(5000, 51)
    with _plan() as plan:
        for s, (D, T) in enumerate([(8, 65), (3, 25), (200, 1601)]):
            plan.tap_open(s, 0.0731 * (s + 1), D)
        plan.tap_reset(n0)
        assert plan.tap_state() == n0 and plan.tap_info(0)["n_open"] == n0
        a = plan.tap_push(x[:2777])
        b = plan.tap_push(x[2777:])
        assert plan.tap_state() == n0 + 5000
    for s, (D, T) in enumerate([(8, 65), (3, 25), (200, 1601)]):
        h = _design(D, T)
        y = np.concatenate([a[s], b[s]])
        ref = tp.ref_push(x, n0, tp.freq_word(0.0731 * (s + 1), 1.0), D, h)
        _under(y, ref, tp.gate(h, np.abs(x).max()), f"n0={n0} D={D}")


# ---------------------------------------------------------------- 6. the other input formats
@pytest.mark.parametrize("in_dtype", ["complex32", "cu8", "f32"])
def test_each_other_input_format(in_dtype):
    D, T, n = 8, 65, 2 * 512 + 301
    z = tp.noise_and_tones(n, 61)
    if in_dtype == "complex32":
        raw = np.stack([z.real, z.imag], axis=1).astype(np.float16).reshape(-1)
    elif in_dtype == "cu8":
        raw = np.clip(np.round(np.stack([z.real, z.imag], axis=1) / 1.5 * 127.5 + 127.5), 0, 255).astype(np.uint8).reshape(-1)
    else:
        raw = z.real.astype(np.float32)
    x = tp.loader(raw, in_dtype)                     # the float32 values the loader defines
    h = _design(D, T)
    with _plan(in_dtype=in_dtype) as plan:
        plan.tap_open(0, 0.0731, D)
        a = plan.tap_push(raw[:2 * 333] if in_dtype in ("complex32", "cu8") else raw[:333])
        b = plan.tap_push(raw[2 * 333:] if in_dtype in ("complex32", "cu8") else raw[333:])
    _under(np.concatenate([a[0], b[0]]), tp.ref_push(x, 0, FW, D, h), tp.gate(h, np.abs(x).max()), in_dtype)


def test_flip_input_is_unsupported():
    from pypanadapter_amd import ZoomFFT
    with ZoomFFT(32, 1, 1.0, flip=True) as plan:
        with pytest.raises(NotImplementedError, match="flip_input"):
            plan.set_taps(4, 65)
        with pytest.raises(ValueError, match="taps are off"):
            plan.tap_state()


# ---------------------------------------------------------------- 7. ordering
def test_a_device_push_behind_a_stalled_stream():
    """process_device on A and, right after it, a tap push of the same buffer on B and another on C,
    enqueued while a bounded spin kernel holds A (tests/stall.py): nothing runs ahead of the plan's
    earlier work, no enqueue waits on the host, and both results are right."""
    import torch
    from pypanadapter_amd import ZoomFFT
    streams = stall.streams()
    F, L, N, D, T = 4, 4096, 1024, 8, 65
    x = tp.noise_and_tones(F * L, 71)
    h = _design(D, T)
    half = F * L // 2

    def bufs():
        return {"x": torch.from_numpy(x.view(np.float32).reshape(F, L, 2).copy()).to("cuda"),
                "rows": stall.sentinel((F, N)), "y": stall.sentinel((F * L // D, 2))}

    def seq(plan, run, b):
        run.call("process", plan.process_device, b["x"].data_ptr(), L, F, b["rows"].data_ptr(), on=streams[0])
        run.call("tap_push0", plan.tap_push_device, b["x"].data_ptr(), half, b["y"].data_ptr(), on=streams[1])
        run.call("tap_push1", plan.tap_push_device, b["x"].data_ptr() + 8 * half, F * L - half,
                 b["y"].data_ptr() + 8 * (half // D), on=streams[2])

    def make():
        plan = ZoomFFT(N, 1, 1.0)
        plan.set_taps(2, T)
        plan.tap_open(0, 0.0731, D, taps=h)
        seq(plan, stall.Run(plan, streams, held=False), bufs())   # the workspaces have their size
        torch.cuda.synchronize()
        plan.tap_reset(0)
        torch.cuda.synchronize()
        return plan, bufs()

    def sequence(plan, run, b):
        seq(plan, run, b)
        run.check_order()
        return {"rows": b["rows"], "y": b["y"]}

    held, stepped, run = stall.enqueue_twice("tap[push]", make, sequence, streams)
    assert run.final_held and run.quiesce_delta == 0             # no host wait in any enqueue
    stall.same_bytes(held, stepped, "held")
    assert not (held["rows"] == stall.SENTINEL).any()
    y = np.ascontiguousarray(held["y"]).view(np.complex64).reshape(-1)
    _under(y, tp.ref_push(x, 0, FW, D, h), tp.gate(h, np.abs(x).max()), "device pushes")
    with ZoomFFT(N, 1, 1.0) as plan:
        np.testing.assert_allclose(plan.rows(x.reshape(F, L)), held["rows"], rtol=0, atol=1e-3)


# ---------------------------------------------------------------- 8. off means off, calls and errors
def test_off_means_off():
    from pypanadapter_amd import ZoomFFT, synth
    x = np.stack([synth.make_iq(65536, 2.4e6, 3 + f, n_fft=1024, zoom=8, n_win=128) for f in range(16)])
    with ZoomFFT(1024, 8, 2.4e6, n_win=128) as plan:
        plan.set_timing(True)
        rows = plan.rows(x)
        names = plan.launch_names()
        assert names and not [n for n in names if "tap" in n]
        for call in (plan.tap_state, plan.tap_shape, lambda: plan.tap_counts(5), lambda: plan.tap_push(x[0]),
                     lambda: plan.tap_close(0), lambda: plan.tap_info(0), plan.tap_reset,
                     lambda: plan.tap_open(0, 0.0, 8), lambda: plan.tap_push_device(8, 1, 8)):
            with pytest.raises(ValueError, match="taps are off"):
                call()
        plan.set_taps(2, 65)                         # on: a process call is still the plan's alone
        plan.tap_open(0, 1e5, 8)
        assert np.array_equal(plan.rows(x), rows) and plan.launch_names() == names
        (y,) = plan.tap_push(x[0])
        assert plan.launch_names() == ["tap_push"] and len(plan.timings()) == 1 and y.size == 65536 // 8
        plan.set_taps(0, 0)                          # off again, everything freed
        with pytest.raises(ValueError, match="taps are off"):
            plan.tap_shape()
        assert np.array_equal(plan.rows(x), rows) and plan.launch_names() == names
        plan.set_taps(0, 0)


def test_calls_and_errors():
    from pypanadapter_amd import _lib
    h = np.float32([0.5, 0.5])
    with _plan(max_taps=3, max_len=65) as plan:
        assert plan.tap_shape() == (3, 65) and plan.tap_state() == 0
        assert plan.tap_counts(100).tolist() == [0, 0, 0] and plan.tap_push(np.zeros(10, np.complex64)) == []
        for bad in [dict(slot=-1), dict(slot=3), dict(decim=0), dict(decim=513), dict(taps=np.zeros(66, np.float32)),
                    dict(taps=np.zeros(0, np.float32))]:
            kw = dict(slot=0, f_hz=0.1, decim=4, taps=h)
            kw.update(bad)
            with pytest.raises(ValueError):
                plan.tap_open(**kw)
        p = h.ctypes.data_as(ctypes.c_void_p)
        assert plan.lib.zfft_tap_open(plan._plan, 0, 2 ** 31, 4, 2, p) == _lib.ZFFT_EINVAL
        assert plan.lib.zfft_tap_open(plan._plan, 0, -2 ** 31 - 1, 4, 2, p) == _lib.ZFFT_EINVAL
        assert plan.lib.zfft_tap_open(plan._plan, 0, 0, 4, 2, None) == _lib.ZFFT_EINVAL
        assert b"tap_open" in plan.lib.zfft_last_error()
        with pytest.raises(ValueError, match="not open"):
            plan.tap_close(0)
        for s in (-1, 3):
            with pytest.raises(ValueError, match="slot"):
                plan.tap_close(s)
            with pytest.raises(ValueError, match="slot"):
                plan.tap_info(s)
        assert plan.tap_info(1) == {"open": False, "freq_word": 0, "f_hz": 0.0, "decim": 0, "n_taps": 0, "n_open": 0,
                                    "group_delay": 0.0}
        f = plan.tap_open(1, 0.25, 4, taps=h)                       # (fs = 1)
        assert f == 0.25 and plan.tap_info(1)["freq_word"] == 2 ** 30 and plan.tap_freq_word(-0.5) == -2 ** 31
        assert plan.tap_freq_word(0.5) == -2 ** 31                  # wrapped into [-2^31, 2^31)
        assert plan.tap_open(0, 0.1, 16) > 0 and plan.tap_info(0)["n_taps"] == 65   # 8 D + 1 capped at max_len
        for n in (-1, 2 ** 31):
            with pytest.raises(ValueError):
                plan.tap_counts(n)
            with pytest.raises(ValueError):
                plan.tap_push_device(8, n, 8)
        with pytest.raises(ValueError, match="null"):
            plan.tap_push_device(0, 5, 8)
        with pytest.raises(ValueError, match="null"):
            plan.tap_push_device(8, 5, 0)
        plan.tap_push_device(0, 0, 0)                               # n_samples = 0: OK, nothing happens
        assert plan.tap_push(np.zeros(0, np.complex64))[0].size == 0 and plan.tap_state() == 10
        for n0 in (-1, 2 ** 62 + 1):
            with pytest.raises(ValueError):
                plan.tap_reset(n0)
        plan.tap_reset(2 ** 62 - 3)
        with pytest.raises(ValueError, match="2\\^62"):
            plan.tap_push(np.zeros(10, np.complex64))
        for bad in [(0, 5), (5, 0), (65, 5), (-1, 5), (4, 2049)]:
            with pytest.raises(ValueError):
                plan.set_taps(*bad)
        assert plan.tap_shape() == (3, 65)                          # a refused call changes nothing
        plan.set_taps(2, 9)                                         # a new shape: every tap closed, the count at 0
        assert plan.tap_shape() == (2, 9) and plan.tap_state() == 0 and not plan.tap_info(1)["open"]


# ---------------------------------------------------------------- 9. the loop closed
def test_a_track_becomes_a_tap():
    """Two tones 1 kHz apart beside a full-scale carrier: the detector and the tracker find the pair,
    Tap.open_for opens on the track's extent, and the tap hands back the pair at -/+ 500 Hz with the
    carrier down by the design's own stopband (measured on the carrier alone: the tap is linear)."""
    from pypanadapter_amd import Detector, Tap, psd_lines, synth
    fs, N, rows = 512e3, 1024, 300
    f_pair, f_car, amp = 60e3, -150e3, 0.1
    n = (rows + 1) * N // 2
    x = synth.tone_pair(n, fs, 81, f_centre=f_pair, spacing=1e3, amp=amp, carrier=(f_car, 1.0), noise=2e-3)
    lines = psd_lines(x, fs, N, 1, 1, window="blackmanharris")
    assert lines.shape == (rows, N)
    det = Detector(threshold_db=40.0, min_width=2, track=(1, 1, 50))   # row units: 20 dB in power
    try:
        det.update(lines)
        op = det.open_tracks()
        ext = det.track_extent(op, fs, N, 1, line_period=0.5 * N / fs)
    finally:
        det.close()
    assert len(op) == 2                               # the carrier and the pair, both still on the air
    i = int(np.argmin(np.abs(ext["f_peak"] - f_pair)))
    assert ext["f_lo"][i] < f_pair - 500 < f_pair + 500 < ext["f_hi"][i] and op["row_first"][i] == 0
    taps = Tap(fs, max_taps=2)
    try:
        slot = taps.open_for(ext, i)
        info = taps.info(slot)
        width = ext["f_hi"][i] - ext["f_lo"][i]
        D, T = info["decim"], info["n_taps"]
        assert fs / D >= 1.25 * width > fs / (D + 1) and T == min(8 * D + 1, 2048) and taps.rate(slot) == fs / D
        y = np.concatenate([taps.push(x[:n // 3])[slot], taps.push(x[n // 3:])[slot]])
    finally:
        taps.close()
    from pypanadapter_amd import tap_design
    h = tap_design(T, 0.4 / D, 8.0).astype(np.float32)
    gate = tp.gate(h, np.abs(x).max())
    _under(y, tp.ref_push(x, 0, info["freq_word"], D, h), gate, "track -> tap")
    # its spectrum: the two tones where they lie from the frequency used, -/+ 500 Hz on the nose when
    # the run is centred on the pair
    skip = T // D + 1                                  # (past the filter's start)
    w = np.blackman(y.size - skip) * np.kaiser(y.size - skip, 20.0)
    w /= w.sum()
    m = np.arange(y.size - skip)

    def level(v, f=None):
        """|the windowed projection of v onto exp(2 pi i f m D / fs)|; f: the carrier's offset by default."""
        f = f_car - info["f_hz"] if f is None else f
        return abs(np.sum(w * np.asarray(v[skip:], dtype=np.complex128) * np.exp(-2j * np.pi * f / (fs / D) * m)))

    H = lambda f: abs(np.sum(h.astype(np.float64) * np.exp(-2j * np.pi * f / fs * np.arange(T))))
    for side in (-500.0, 500.0):
        f = f_pair + side - info["f_hz"]
        assert abs(abs(f) - 500.0) <= 0.5 * fs / N + 1e-9   # the centre is right to half a bin: the extent's grid
        got = level(y, f)
        print(f"tone at {f:+.1f} Hz: {got:.5f} (amp {amp} x |H| {H(f):.5f})")
        assert abs(got - amp * H(f)) <= 1e-3 * amp
    # the carrier: down by the design's stopband |H| at its offset, a number from the taps alone.
    # The tap is linear, so the carrier is measured on its own: the same stream without the pair and
    # without the noise, through the same tap on a fresh plan.  The float64 reference of that stream
    # sits at |H| (the window's leakage is far below it); float32 arithmetic moves single outputs
    # by some 1e-8 here and the windowed sum averages that down, so |H| once more is ample room.
    off = f_car - info["f_hz"]
    want = 1.0 * H(off)
    xc = synth.tone_pair(n, fs, 81, f_centre=f_pair, spacing=1e3, amp=0.0, carrier=(f_car, 1.0), noise=0.0)
    alone = Tap(fs, max_taps=2)
    try:
        assert alone.open(slot, info["f_hz"], D) == info["f_hz"] and alone.info(slot)["n_taps"] == T
        yc = np.concatenate([alone.push(xc[:n // 3])[slot], alone.push(xc[n // 3:])[slot]])
    finally:
        alone.close()
    ref_c = tp.ref_push(xc, 0, info["freq_word"], D, h)
    _under(yc, ref_c, tp.gate(h, np.abs(xc).max()), "carrier alone")
    got_c, ref_level = level(yc), level(ref_c)
    print(f"carrier alone at {off:+.1f} Hz from the tap: {got_c:.4e}; float64 reference {ref_level:.4e}; "
          f"|H| = {want:.4e} ({20 * np.log10(want):.1f} dB)")
    assert want < 1e-5 and abs(ref_level - want) <= 1e-3 * want and got_c <= 2.0 * want
    # in the whole scene the figure at that offset is higher, and the excess is the scene's own
    # in-band noise (and the pair's skirt), not the carrier and not float32: the float64 reference
    # of the scene without its carrier accounts for it
    rest = level(tp.ref_push(x.astype(np.complex128) - xc.astype(np.complex128), 0, info["freq_word"], D, h))
    got = level(y)
    print(f"whole scene at {off:+.1f} Hz: {got:.3e}; the scene without its carrier (float64): {rest:.3e}")
    assert got <= 2.0 * want + rest
