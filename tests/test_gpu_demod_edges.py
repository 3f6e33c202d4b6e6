"""GPU checks of the demodulator bank's code no other test reaches (zfft_plan_demod;
csrc/demod_kernels.hip): FM between 0.9 pi and its branch at +-pi, input strides other than (K, 1),
(1, steps) and (1, 0) -- pitched, interleaved, overlapping, past 4 GiB in bytes -- a push of more
tiles than the grid has workgroups, and the largest span.  Wherever AM, POWER or SSB at a
quarter-turn word serves, the comparison is with demod_ref's float32 model, value for value
(dr.same: NaN equal to NaN, +0 to -0, no tolerance); pushes of one signal through two layouts are
compared bytewise; FM's detector goes against the float64 reference."""
import numpy as np
import pytest

import demod_ref as dr
import f32_exact as fx
import stall
from test_demod_host import demod_form
from test_gpu_demod import _dev, _plan, _push, _words

pytestmark = pytest.mark.gpu
QUARTER = np.array(dr.QUARTER_WORDS, dtype=np.int64)
NAN = np.complex64(complex(np.nan, np.nan))


@pytest.fixture(scope="module", autouse=True)
def _gpu(zfft_lib):
    from pypanadapter_amd import device_count
    assert device_count() >= 1, "GPU tests need a HIP device"


def equal(got, want, what):
    assert dr.same(got, want), f"{what}: {dr.first_difference(got, want)}"


def mixed(K, seed):
    """Modes going round AM, FM, SSB, POWER; every second SSB stream at a quarter-turn word."""
    modes, words = np.arange(K) % 4, _words(K, seed)
    ssb = np.nonzero(modes == dr.SSB)[0]
    words[ssb[::2]] = QUARTER[1 + np.arange(ssb[::2].size) % 3]
    return modes, words


def model_of(a, x, n0, modes, words, g, Da, what):
    """The streams the host models, against the model."""
    host = np.array([dr.modelled(m, w) for m, w in zip(modes, words)])
    assert host.any()
    equal(a[:, host], dr.model_push(x[:, host], n0, modes[host], words[host], g, Da), what)


# ---------------------------------------------------------------- 1. FM up to the branch
def branch_signal(n, K, seed):
    """(n, K) complex64 of constant envelope whose phase steps are drawn over [-pi, pi], with steps
    within a few 2^-24 of +-pi on both sides, steps of exactly pi (x[n] = -x[n - 1]), and stretches
    on the real axis and on the diagonal with components that are powers of two, where the products
    are exact and z.im is +0 or -0 with z.re < 0."""
    rng = np.random.default_rng(seed)
    step = rng.uniform(-np.pi, np.pi, (n, K))
    near = rng.random((n, K)) < 0.2
    step = np.where(near, rng.choice([-1.0, 1.0], (n, K)) * np.pi * (1.0 - rng.integers(0, 9, (n, K)) * 2.0 ** -24), step)
    x = (rng.uniform(0.5, 1.5, K) * np.exp(1j * np.cumsum(step, axis=0))).astype(np.complex64)
    for i in range(40, n - 40, 97):                       # x[n] = -x[n - 1] in float32, three in a row
        for j in range(3):
            x[i + j] = -x[i + j - 1]
    sign = np.where(np.arange(12) % 2, -1.0, 1.0)[:, None]
    x[200:212] = sign * 0.75                              # the real axis: z = (-0.5625, -+0)
    x[300:312] = -sign * 0.75
    x[400:412] = sign * (0.5 + 0.25j)                     # exact products: z.im = +-0 again
    x[500:512] = sign * (-0.25 + 2.0j)
    return x


def test_fm_between_0_9_pi_and_the_branch():
    """Prints the worst |d - d_ref| on the samples with |arg z| <= 0.9 pi (asserted under the header's
    EPS_FM 2^-24) and, modulo 2, on the samples beyond, up to the branch (asserted under 16 2^-24,
    the header's own condition on EPS_FM; the figure is in profiles/demod/README.md).  Where z.im is
    +-0 and z.re < 0 in float32, d is mul(+-float32(pi), float32(1 / pi)) exactly."""
    K, n = 8, 4096
    x = branch_signal(n, K, 3)
    with _plan(K, 1, 1, np.float32([1.0]), dr.FM) as plan:
        d = _push(plan, x)
    x64 = x.astype(np.complex128)
    z = x64[1:] * np.conj(x64[:-1])                       # float32 products are exact in float64
    ref = np.angle(z) / np.pi
    got = d[1:].astype(np.float64)
    inside = np.abs(np.angle(z)) <= dr.FM_ARG_MAX * np.pi
    e_in = np.abs(got - ref)[inside].max()
    e_out = np.abs((got - ref + 1.0) % 2.0 - 1.0)[~inside].max()
    close = np.abs(np.abs(np.angle(z)) - np.pi) <= 16 * np.pi * dr.U
    print(f"FM detector: worst |d - d_ref| = {e_in / dr.U:.3f} x 2^-24 on {int(inside.sum())} samples inside 0.9 pi; "
          f"modulo 2, {e_out / dr.U:.3f} x 2^-24 on {int((~inside).sum())} samples beyond it, "
          f"{int(close.sum())} of them within 16 x 2^-24 pi of the branch")
    assert inside.sum() > 1000 and (~inside).sum() > 1000 and close.sum() > 500
    assert e_in <= dr.EPS_FM * dr.U
    assert e_out <= 16 * dr.U
    assert (got[close] > 0.99).any() and (got[close] < -0.99).any() and np.abs(got).max() <= 1.0 + 2 * dr.U
    # exactly on the branch
    z_re, z_im = dr.fm_z_f32(x)
    on = (z_im == 0) & (z_re < 0)
    assert (on & np.signbit(z_im)).sum() >= 16 and (on & ~np.signbit(z_im)).sum() >= 16
    pi, inv_pi = np.float32(np.pi), np.float32(1.0 / np.pi)
    want = fx.mul(np.where(np.signbit(z_im[on]), -pi, pi).astype(np.float32), np.full(int(on.sum()), inv_pi, np.float32))
    assert d[on].tobytes() == want.tobytes(), dr.first_difference(d[on], want)


# ---------------------------------------------------------------- 2. strides
def strided_push(plan, x, ss, ts, offset=0, cut=None, guard=64):
    """x (steps, K) laid out at complex index offset + n ss + s ts in a buffer that is NaN everywhere
    else (the gaps, `offset` before and `guard` behind: a read outside the rule's positions shows in
    the audio), pushed from the device in pieces of `cut`; (outputs, K) float32, nothing written
    beyond them."""
    import torch
    n, K = x.shape
    idx = offset + np.arange(n)[:, None] * ss + np.arange(K)[None, :] * ts
    buf = np.full(int(idx.max()) + 1 + guard, NAN, np.complex64)
    buf[idx] = x
    assert np.array_equal(buf[idx], x)                    # (overlapping strides: x must agree with itself)
    d_x = _dev(buf)
    parts, at = [], 0
    for c in ([n] if cut is None else cut):
        outs = plan.demod_steps(c)
        d_a = stall.sentinel((outs * K + guard,))
        plan.demod_push_device(d_x.data_ptr() + 8 * (offset + at * ss), c, ss, ts, d_a.data_ptr())
        torch.cuda.synchronize()
        a = d_a.cpu().numpy()
        assert (a[outs * K:] == stall.SENTINEL).all()
        parts.append(a[:outs * K].reshape(outs, K).copy())
        at += c
    assert at == n
    return np.concatenate(parts)


STRIDED = {  # name: (K, step_stride, stream_stride, offset, kind, stream_tiles); a stride of None is steps + 13
    "subset-in-place-streams": (8, 64, 1, 5, 1, 1),
    "subset-in-place-time": (5, 64, 1, 5, 0, 5),
    "every-second-column": (8, 64, 2, 5, 0, 8),
    "time-layout-with-a-pitch": (3, 1, None, 3, 0, 3),
    "overlapping-streams": (8, 1, 1, 2, 1, 1),
    "overlapping-time": (3, 1, 1, 2, 0, 3),
    "one-stream-step-1": (1, 1, 0, 7, 0, 1),
    "one-stream-step-7": (1, 7, 0, 7, 0, 1),
}


@pytest.mark.parametrize("name", list(STRIDED))
def test_strided_input_is_the_same_signal_pushed_as_K_1(name):
    K, ss, ts, offset, kind, tiles = STRIDED[name]
    Ta, Da = 33, 4
    g = dr.audio_taps(Ta, Da)
    modes, words = mixed(K, 40)
    with _plan(K, Ta, Da, g, modes, words) as plan:
        span = demod_form(plan.lib, K, Ta, Da, ss, ts or 99999)["span"]
        n = 2 * span + 77 if kind else span + 501       # more than one span in either form
        ts = n + 13 if ts is None else ts
        f = demod_form(plan.lib, K, Ta, Da, ss, ts, 0, n)
        assert (f["kind"], f["stream_tiles"]) == (kind, tiles) and f["nspans"] >= 2
        if "overlapping" in name:                         # stream s is one sequence, s steps on
            seq = dr.fm_signal(n + K - 1, 1, 41)[:, 0]
            x = np.stack([seq[s:s + n] for s in range(K)], axis=1)
        else:
            x = dr.fm_signal(n, K, 41)
        want = _push(plan, x, "streams")                  # the same signal as (K, 1)
        plan.demod_reset(0)
        a = strided_push(plan, x, ss, ts, offset)
        plan.demod_reset(0)
        b = strided_push(plan, x, ss, ts, offset, cut=[span - 1, Ta - 1, n - span - Ta + 2])
    assert a.tobytes() == want.tobytes(), dr.first_difference(a, want)
    assert b.tobytes() == want.tobytes(), dr.first_difference(b, want)
    assert np.isfinite(want).all()
    model_of(a, x, 0, modes, words, g, Da, name)


# ---------------------------------------------------------------- 3. offsets past 4 GiB
FAR = {"two-streams-2^29+5-apart": (2, 1, 2 ** 29 + 5, 300, 0), "eight-streams-steps-2^17+1-apart": (8, 2 ** 17 + 1, 1, 4200, 1),
       "one-stream-steps-2^17+1-apart": (1, 2 ** 17 + 1, 0, 4200, 0)}


@pytest.mark.parametrize("name", list(FAR))
def test_offsets_past_4_gib(name):
    """Strides that take the last sample more than 2^32 bytes from the first (4.29 GB and 4.40 GB):
    the buffer comes from torch.empty, only the positions the call reads are written, on the device,
    and it is freed before the test returns.  The audio is that of the same signal pushed as (K, 1),
    bytewise, and the model's.  A stride of 2^31 itself, the largest rule 0 allows, needs 16 GiB per
    step or stream and is left out."""
    import torch
    K, ss, ts, n, kind = FAR[name]
    Ta, Da = 33, 4
    g = dr.audio_taps(Ta, Da)
    modes, words = mixed(K, 42)
    x = dr.fm_signal(n, K, 43)
    idx = np.arange(n)[:, None] * ss + np.arange(K)[None, :] * ts
    assert 8 * int(idx.max()) > 2 ** 32 and 8 * (int(idx.max()) + 1) < 4.5e9
    with _plan(K, Ta, Da, g, modes, words) as plan:
        assert demod_form(plan.lib, K, Ta, Da, ss, ts, 0, n)["kind"] == kind
        want = _push(plan, x, "streams")
        plan.demod_reset(0)
        outs = plan.demod_steps(n)
        d_a = stall.sentinel((outs * K + 64,))
        buf = torch.empty(int(idx.max()) + 1, dtype=torch.complex64, device="cuda")     # the one allocation
        try:
            buf[torch.from_numpy(idx.reshape(-1)).to("cuda")] = torch.from_numpy(x.reshape(-1).copy()).to("cuda")
            plan.demod_push_device(buf.data_ptr(), n, ss, ts, d_a.data_ptr())
            torch.cuda.synchronize()
        finally:
            del buf
            torch.cuda.empty_cache()
        a = d_a.cpu().numpy()
    assert (a[outs * K:] == stall.SENTINEL).all()
    a = a[:outs * K].reshape(outs, K)
    assert a.tobytes() == want.tobytes(), dr.first_difference(a, want)
    model_of(a, x, 0, modes, words, g, Da, name)


# ---------------------------------------------------------------- 4. more tiles than workgroups
def test_more_tiles_than_workgroups():
    """The smallest push whose tiles outnumber the grid's 65536 workgroups: K = 1024, Ta = 65,
    Da = 64 is the streams form at 64 lanes, span 64, 16 stream tiles, and 4097 spans are 65552
    tiles, so sixteen workgroups take a second tile -- tile 65536 is span 4096 of stream tile 0.  The
    last span is ragged (41 steps).  2.15 GB of input from a seeded generator on the device; AM
    against the model on four whole streams and, for the spans 0, 1, 4095 and 4096, on every
    stream."""
    import torch
    K, Ta, Da = 1024, 65, 64
    n = 4096 * 64 + 41
    g = dr.audio_taps(Ta, Da)
    with _plan(K, Ta, Da, g) as plan:
        f = demod_form(plan.lib, K, Ta, Da, K, 1, 0, n)
        assert (f["kind"], f["lanes"], f["span"], f["stream_tiles"], f["nspans"]) == (1, 64, 64, 16, 4097)
        assert f["ntiles"] == 65552 > f["grid"] == 65536 and n % f["span"] == 41
        outs = plan.demod_steps(n)
        assert outs == 4097
        gen = torch.Generator(device="cuda").manual_seed(7)
        d_x = torch.randn((n, K, 2), generator=gen, device="cuda", dtype=torch.float32)
        d_x *= 0.5
        d_a = stall.sentinel((outs * K + 64,))
        plan.demod_push_device(d_x.data_ptr(), n, K, 1, d_a.data_ptr())
        torch.cuda.synchronize()
        a = d_a.cpu().numpy()
        whole = [0, 337, 700, 1023]
        x_whole = np.ascontiguousarray(d_x[:, whole].cpu().numpy()).view(np.complex64).reshape(n, len(whole))
        rows = {m: np.ascontiguousarray(d_x[max(0, m * Da - Ta + 1):m * Da + 1].cpu().numpy()).view(np.complex64).reshape(-1, K)
                for m in (0, 1, 4095, 4096)}
        del d_x
        torch.cuda.empty_cache()
    assert (a[outs * K:] == stall.SENTINEL).all()
    a = a[:outs * K].reshape(outs, K)
    for m, x in rows.items():                             # output m is span m's one output, step 64 m
        first = max(0, m * Da - Ta + 1)
        equal(a[m:m + 1], dr.fir_f32(dr.am_f32(x), g, Da, m * Da, 1, first=first), f"span {m}, every stream")
    equal(a[:, whole], dr.fir_f32(dr.am_f32(x_whole), g, Da, 0, n), "four whole streams")
    assert np.isfinite(a).all() and a.std() > 0.1


# ---------------------------------------------------------------- 5. the largest span
def test_the_largest_span():
    """Time form, K = 3, Ta = 33, Da = 4: span 8192, the largest.  Five spans and a ragged tail, AM,
    every output against the model -- the outputs around every span boundary first."""
    K, Ta, Da = 3, 33, 4
    n = 5 * 8192 + 77
    g = dr.audio_taps(Ta, Da)
    x = dr.noise_and_tones(n, K, 45)
    with _plan(K, Ta, Da, g) as plan:
        f = demod_form(plan.lib, K, Ta, Da, 1, n, 0, n)
        assert (f["kind"], f["span"], f["nspans"], f["ntiles"]) == (0, 8192, 6, 18)
        a = _push(plan, x, "time")
    want = dr.model_push(x, 0, dr.AM, 0, g, Da)
    for b in range(1, 6):
        m = np.arange(b * 8192 // Da - 12, b * 8192 // Da + 12)
        equal(a[m], want[m], f"around the boundary of spans {b - 1} and {b}")
    equal(a, want, "span 8192")
