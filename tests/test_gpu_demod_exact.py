"""GPU checks of the demodulator bank (zfft_plan_demod; csrc/demod_kernels.hip) against the header's
arithmetic itself: demod_ref's float32 model (detect_f32, fir_f32 on tests/f32_exact.py) rounds
where rules 2 and 3 of include/zfft.h say the kernel rounds, so every comparison here is
`np.array_equal(got, want, equal_nan=True)` on float32 -- +0 equal to -0, because the header does
not fix the sign of a zero sum, and no tolerance.

AM, POWER and SSB at the four quarter-turn words are modelled wholly on the host.  FM and SSB at a
general word call device library functions (atan2f, sincospif) the host cannot reproduce: their
detected values come from a second plan with Ta = 1, g = [1], Da = 1 at the same count, modes and
words, whose output is the detected value itself, and fir_f32 runs on them -- the filter, the
indexing, the carry and the decimation are pinned exactly and only the library call stays outside.
Every comparison counts its values (`COMPARED`; the session's total is in profiles/demod)."""
import functools

import numpy as np
import pytest

import demod_ref as dr
from test_gpu_demod import _form, _plan, _push, _signal, _words

pytestmark = pytest.mark.gpu
COMPARED = [0]
QUARTER = np.array(dr.QUARTER_WORDS, dtype=np.int64)


@pytest.fixture(scope="module", autouse=True)
def _gpu(zfft_lib):
    from pypanadapter_amd import device_count
    assert device_count() >= 1, "GPU tests need a HIP device"
    yield
    print(f"\nexact comparisons of the bank: {COMPARED[0]} values, none differing")


def equal(got, want, what):
    """got == want value for value (dr.same), counted; the first difference with its bits otherwise."""
    assert dr.same(got, want), f"{what}: {dr.first_difference(got, want)}"
    COMPARED[0] += int(np.asarray(want).size)


def push_cut(plan, x, layout, cut=None):
    """x pushed in pieces of `cut` steps (None: one push); the outputs back to back."""
    parts, at = [], 0
    for c in ([len(x)] if cut is None else cut):
        parts.append(_push(plan, x[at:at + c], layout))
        at += c
    assert at == len(x)
    return np.concatenate(parts)


def detected(x, n0, modes, words, layout="streams"):
    """d[i, s] in float32 for the (steps, K) stream at count n0: the host's model where it has one,
    and for the other streams what the device detects -- a plan of Ta = 1, g = [1], Da = 1, whose
    output fma(1, d, +0) is d.  Where both exist they are compared on the way."""
    K = x.shape[1]
    modes = np.broadcast_to(np.asarray(modes, dtype=np.int64), (K,))
    words = np.broadcast_to(np.asarray(words, dtype=np.int64), (K,))
    host = np.array([dr.modelled(m, w) for m, w in zip(modes, words)])
    d = np.zeros(x.shape, np.float32)
    if not host.all():
        with _plan(K, 1, 1, np.float32([1.0]), modes, words) as plan:
            plan.demod_reset(n0)
            d = _push(plan, x, layout)
        assert d.shape == x.shape
    if host.any():
        model = dr.detect_f32(x[:, host], n0, modes[host], words[host])
        if not host.all():
            equal(d[:, host], model, "the detected values of the modelled streams")
        d[:, host] = model
    return d


def want_push(x, n0, modes, words, g, Da, layout="streams"):
    return dr.fir_f32(detected(x, n0, modes, words, layout), g, Da, n0, len(x))


# ---------------------------------------------------------------- 1. every case, every mode
@pytest.mark.parametrize("mode", ["am", "fm", "ssb", "power", "ssb-quarter"])
@pytest.mark.parametrize("i", range(len(dr.CASES)), ids=dr.IDS)
def test_each_mode_is_the_float32_rule(i, mode):
    K, Ta, Da, layout = dr.CASES[i]
    m = dr.MODES[mode.split("-")[0]]
    g = dr.audio_taps(Ta, Da)
    words = QUARTER[np.arange(K) % 4] if mode == "ssb-quarter" else _words(K, 100 + i) if m == dr.SSB else np.zeros(K, np.int64)
    with _plan(K, Ta, Da, g, m, words) as plan:
        n = dr.case_len(_form(plan, layout)["span"])
        x = _signal(i, m == dr.FM, n)
        a = _push(plan, x, layout)
    assert all(dr.modelled(m, w) for w in words) == (mode in ("am", "power", "ssb-quarter"))
    equal(a, want_push(x, 0, m, words, g, Da, layout), f"{dr.IDS[i]} {mode}")


# ---------------------------------------------------------------- 2. both forms
def test_both_forms_are_the_float32_rule():
    """The mixed-mode case of test_gpu_demod.test_both_forms_give_the_same_bits, the carry going from
    one form to the other, against the model in both orders."""
    K, Ta, Da = 64, 65, 8
    g = dr.audio_taps(Ta, Da)
    modes, words = np.arange(K) % 4, _words(K, 70)
    words[2::8] = QUARTER[np.arange(K // 8) % 4]          # every second SSB stream at a quarter-turn word
    x = dr.fm_signal(1500, K, 35)
    with _plan(K, Ta, Da, g, modes, words) as plan:
        assert _form(plan, "streams")["kind"] == 1 and _form(plan, "time")["kind"] == 0
        ab = np.concatenate([_push(plan, x[:700], "streams"), _push(plan, x[700:], "time")])
        plan.demod_reset(0)
        cd = np.concatenate([_push(plan, x[:333], "time"), _push(plan, x[333:], "streams")])
    want = want_push(x, 0, modes, words, g, Da)
    equal(ab, want, "streams then time")
    equal(cd, want, "time then streams")


# ---------------------------------------------------------------- 3. cuts and a count past 2^32, one case per form
@pytest.mark.parametrize("K,Ta,Da,layout", [(64, 65, 8, "streams"), (5, 33, 4, "time")], ids=["streams", "time"])
def test_cuts_and_a_late_count_are_the_float32_rule(K, Ta, Da, layout):
    g = dr.audio_taps(Ta, Da)
    modes, words = np.arange(K) % 4, _words(K, 60)
    words[modes == dr.SSB] = np.where(np.arange((modes == dr.SSB).sum()) % 2, QUARTER[1], words[modes == dr.SSB])
    n0 = 2 ** 32 - 100                                   # the count wraps inside the push: SSB's phase is mod 2^32
    with _plan(K, Ta, Da, g, modes, words) as plan:
        f = _form(plan, layout)
        span = f["span"]
        assert f["kind"] == (1 if layout == "streams" else 0)
        cut = [1, Da - 1, Ta - 1, Ta, span - 1, span + 1, 1]
        n = sum(cut) + span + 5
        cut.append(n - sum(cut))
        x = dr.fm_signal(n, K, 38)
        got = {}
        for start in (0, n0):
            plan.demod_reset(start)
            got[start, "whole"] = push_cut(plan, x, layout)
            plan.demod_reset(start)
            got[start, "cut"] = push_cut(plan, x, layout, cut)
            assert plan.demod_state() == start + n
    for start in (0, n0):
        want = want_push(x, start, modes, words, g, Da, layout)
        equal(got[start, "whole"], want, f"{layout} whole at {start}")
        equal(got[start, "cut"], want, f"{layout} cut at {start}")


# ---------------------------------------------------------------- 4. special values
BIG = [2.0 ** 64, 3 * 2.0 ** 126]                        # their power overflows
FAMILY = [0.0, -0.0, 2.0 ** -149, 2.0 ** -75, 2.0 ** -64, 1.0, 2.0 ** 63] + BIG


@functools.lru_cache(maxsize=None)
def special_streams(n, K, seed=5):
    """(n, K) complex64 whose components are drawn from FAMILY with random signs (the two overflowing
    ones seldom, so that most filter windows stay finite) and from ordinary samples, with stretches
    of a family repeated so that FM meets each against itself."""
    rng = np.random.default_rng(seed)
    p = np.array([4, 4, 6, 6, 6, 6, 3, 0.4, 0.4])
    parts = []
    for _ in range(2):
        pick = rng.choice(len(FAMILY), (n, K), p=p / p.sum())
        hold = rng.random((n, K)) < 0.4                   # repeat the step before: x and p of one family
        for i in range(1, n):
            pick[i] = np.where(hold[i], pick[i - 1], pick[i])
        v = np.array(FAMILY)[pick] * rng.choice([-1.0, 1.0], (n, K))
        parts.append(np.where(rng.random((n, K)) < 0.35, rng.standard_normal((n, K)), v))
    x = (parts[0] + 1j * parts[1]).astype(np.complex64)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("K,layout", [(16, "streams"), (3, "time")], ids=["streams", "time"])
def test_special_values(K, layout):
    """Zeros of both signs, denormals, squares that underflow to zero or into the denormals, squares
    that overflow, among ordinary samples.  AM and POWER equal the model, inf and NaN included: the
    model's clean CPU run is what the header's expression gives.  FM's d is 0 exactly where the
    predicate z.re == z.im == 0 holds in float32 -- x != 0 with both products underflowing included
    -- and elsewhere it is atan2f's value, which is 0 only where the angle itself is: compared with
    the float64 angle of the float32 z (zero where that is zero, non-zero where that is at least
    2^-100, and within the header's 16 2^-24, modulo 2, where z is finite with a component of at
    least 2^-100 so that its roundings are relative ones)."""
    Ta, Da = 9, 2
    g = dr.audio_taps(Ta, Da)
    modes = np.array([dr.AM, dr.POWER, dr.FM] * K)[:K]
    with _plan(K, Ta, Da, g, modes) as plan:
        f = _form(plan, layout)
        assert f["kind"] == (1 if layout == "streams" else 0)
        n = 2 * f["span"] + 37 if layout == "streams" else 1500
        x = special_streams(n, K)
        a = _push(plan, x, layout)
    with _plan(K, 1, 1, np.float32([1.0]), modes) as plan:
        d = _push(plan, x, layout)
    with np.errstate(all="ignore"):
        host = modes != dr.FM
        model = dr.detect_f32(x[:, host], 0, modes[host], 0)
        assert np.isinf(model).any() and (model == 0).any() and ((model > 0) & (model < 2.0 ** -126)).any()
        equal(d[:, host], model, "AM and POWER of the special values")
        dm = d.copy()
        dm[:, host] = model
        want = dr.fir_f32(dm, g, Da, 0, n)
        assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).mean() > 0.5
        equal(a, want, "the audio of the special values")
        # FM
        xf, df = x[:, ~host], d[:, ~host]
        zero = dr.fm_zero_f32(xf)
        prev = np.vstack([np.zeros((1, xf.shape[1]), np.complex64), xf[:-1]])
        assert (zero & (xf != 0) & (prev != 0)).any()     # x and p non-zero, both products underflow
        z_re, z_im = (v.astype(np.float64) for v in dr.fm_z_f32(xf))
        ref = np.arctan2(z_im, z_re) / np.pi
        assert not df[zero].any()
        rest = ~zero
        assert np.array_equal(np.isnan(df[rest]), np.isnan(ref[rest]))
        assert not df[rest & (ref == 0)].any() and (rest & (ref == 0)).any()
        solid = rest & (np.abs(ref) >= 2.0 ** -100)
        assert solid.any() and (df[solid] != 0).all()
        assert (np.abs(df[rest & ~solid & ~np.isnan(ref)]) <= 2.0 ** -99).all()
        close = solid & np.isfinite(z_re) & np.isfinite(z_im) & (np.maximum(np.abs(z_re), np.abs(z_im)) >= 2.0 ** -100)
        err = np.abs((df[close].astype(np.float64) - ref[close] + 1.0) % 2.0 - 1.0).max()
        print(f"FM on the special values ({layout}): {int(zero.sum())} forced zeros, {int(close.sum())} angles, "
              f"worst |d - d_ref| mod 2 = {err / dr.U:.3f} x 2^-24")
        assert err <= 16 * dr.U
    COMPARED[0] += int(zero.sum())


# ---------------------------------------------------------------- 5. NaN containment
@pytest.mark.parametrize("K,layout", [(16, "streams"), (3, "time")], ids=["streams", "time"])
def test_a_nan_or_an_inf_stays_in_its_stream_and_its_window(K, layout):
    Ta, Da = 9, 2
    g = dr.audio_taps(Ta, Da)
    modes, words = np.array([dr.AM, dr.FM, dr.POWER, dr.SSB] * K)[:K], _words(K, 77)
    with _plan(K, Ta, Da, g, modes, words) as plan:
        span = _form(plan, layout)["span"]
        n = span + 300
        p = span - 1                                     # the last step of a span: the window reaches into the next
        base_x = dr.noise_and_tones(n, K, 19)
        base = _push(plan, base_x, layout)
        at = np.arange(base.shape[0]) * Da                # output m is step m Da
        for s in range(min(K, 4)):                        # one stream of each mode
            for bad in (np.nan, np.inf):
                x = base_x.copy()
                x[p, s] = complex(bad, x[p, s].imag)
                plan.demod_reset(0)
                a = push_cut(plan, x, layout, [p + 1, n - p - 1])     # the bad sample goes through the carry
                w = Ta + 1 if modes[s] == dr.FM else Ta
                inside = (at >= p) & (at <= p + w - 1)
                others = np.arange(K) != s
                equal(a[:, others], base[:, others], f"{layout}: the other streams, {bad} in stream {s}")
                equal(a[~inside, s], base[~inside, s], f"{layout}: stream {s} outside the window of its {bad}")
                assert inside.sum() >= Ta // Da and not dr.same(a[inside, s], base[inside, s])
                if not (modes[s] == dr.FM and np.isinf(bad)):     # (FM of an inf is an angle: z = (+-inf, +-inf))
                    assert not np.isfinite(a[inside, s]).any()
                if modes[s] in (dr.AM, dr.POWER):
                    with np.errstate(all="ignore"):
                        want = dr.model_push(x[:, s:s + 1], 0, modes[s], 0, g, Da)
                    assert not np.isfinite(want[inside]).any()
                    equal(a[:, s:s + 1], want, f"{layout}: stream {s} with its {bad}")
