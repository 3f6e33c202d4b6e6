"""CPU checks of the level bank's host side: level_ref's division against exact rationals; emitted()
and the steps of a push against Python integers at late counts and unaligned starts; the model's
prefix stability (so it cannot depend on the cut), rule 6's overshoot bound on adversarial inputs
and the squelch's edges; the form chooser through its hook over a grid and, over its whole domain,
as a stand-alone program under ASan + UBSan (tests/host/level_form_sweep.cpp); the C-ABI's new
names, their ctypes signatures and the errors that need no device."""
import ctypes
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import level_ref as lr
from test_host import header_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["zfft_plan_level", "zfft_level_shape", "zfft_level_steps", "zfft_level_push_device", "zfft_level_push",
         "zfft_level_state", "zfft_level_reset", "zfft_level_info", "zfft_level_meter"]
EINVAL = -1
FORM = ("kind", "lanes", "rows", "chunk", "piece", "lds_bytes", "lane_tiles", "g_lanes", "g_blocks", "g_lds_bytes", "g_lane_tiles",
        "outs", "u_in0", "u_in1", "e0u", "e1u", "nq", "npk", "p_tiles", "g_tiles", "a_tiles", "p_grid", "g_grid", "a_grid")
STARTS = (0, 5, 2 ** 32 - 100, 2 ** 62 - 10 ** 6, 2 ** 62 - 10 ** 6 + 7)
F32 = np.float32


def level_form(lib, K, B, H, n0=0, n_r=0, steps=1):
    """The form dict of zfft__level_form (the shape's form and the cut of a push), or None where it refuses."""
    hook = lib.zfft__level_form
    hook.argtypes = [ctypes.c_int32] * 3 + [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p]
    hook.restype = ctypes.c_int
    form = np.zeros(len(FORM), np.int64)
    if hook(K, B, H, n0, n_r, steps, form.ctypes.data_as(ctypes.c_void_p)):
        return None
    return dict(zip(FORM, map(int, form)))


def lib_emitted(lib, N, n_r, B):
    hook = lib.zfft__level_emitted
    hook.argtypes, hook.restype = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int32], ctypes.c_int64
    return int(hook(N, n_r, B))


def lib_steps(lib, n0, n_r, n, B):
    hook = lib.zfft__level_steps
    hook.argtypes, hook.restype = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int32], ctypes.c_int64
    return int(hook(n0, n_r, n, B))


# ---------------------------------------------------------------- the division
def _round_f32(q):
    """The float32 nearest the positive Fraction q (ties to even), as a Fraction; None where the
    result is not a normal float32."""
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    if not -126 <= e <= 127:
        return None
    ulp = Fraction(2) ** (e - 23)
    k = q / ulp
    n = k.numerator // k.denominator
    rem = k - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    return n * ulp


def test_div_is_correctly_rounded():
    rng = np.random.default_rng(0)
    a = np.concatenate([rng.uniform(0.5, 2.0, 3000) * 2.0 ** rng.integers(-60, 61, 3000), [2.0 ** 60, 2.0 ** -60, 0.5, 0.5, 1.0, 3.0]]).astype(F32)
    b = np.concatenate([rng.uniform(0.5, 2.0, 3000) * 2.0 ** rng.integers(-60, 61, 3000), [2.0 ** -60, 2.0 ** 60, 1e-6, 3.0, 3.0, 1.0]]).astype(F32)
    # quotients on a tie of the 25th bit and next to one: (2^24 + 1 +- d) / 2^24 ...
    a = np.concatenate([a, F32([16777215.0, 16777213.0, 1.0, 1.0])])
    b = np.concatenate([b, F32([16777216.0, 8388607.0, 16777215.0, 8388609.0])])
    got = lr.div(a, b)
    assert got.dtype == F32
    checked = 0
    for x, y, g in zip(a, b, got):
        want = _round_f32(Fraction(float(x)) / Fraction(float(y)))
        if want is not None:
            assert Fraction(float(g)) == want, (x, y, g)
            checked += 1
    assert checked >= 3000
    with np.errstate(all="ignore"):
        assert lr.div(F32([1.0]), F32([0.0]))[0] == np.inf and np.isnan(lr.div(F32([0.0]), F32([0.0]))[0])
    # ... and a reciprocal and a product would differ somewhere: the negative control
    x = rng.uniform(1.0, 2.0, 200000).astype(F32)
    y = rng.uniform(1.0, 2.0, 200000).astype(F32)
    exact = lr.div(x, y)
    recip = (x * (F32(1.0) / y)).astype(F32)              # what a reciprocal would give
    assert (recip != exact).any()


# ---------------------------------------------------------------- the count
def test_emitted_and_steps_at_late_counts_and_unaligned_starts(zfft_lib):
    rng = np.random.default_rng(2)
    for B in (8, 64, 1024):
        for n_r in STARTS:
            for d in (0, 1, B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1, 7 * B + 3, 10 ** 5):
                if n_r + d > 2 ** 62:
                    continue
                want = max(n_r, B * ((n_r + d) // B - 1))
                assert lib_emitted(zfft_lib, n_r + d, n_r, B) == lr.emitted(n_r + d, n_r, B) == want, (B, n_r, d)
            cuts = [int(c) for c in rng.integers(0, 3 * B, 40)]
            at, total = n_r, 0
            for c in cuts:
                got = lib_steps(zfft_lib, at, n_r, c, B)
                assert got == lr.steps(at, n_r, c, B) >= 0
                total += got
                at += c
            assert total == lib_steps(zfft_lib, n_r, n_r, sum(cuts), B) == lr.emitted(at, n_r, B) - n_r
            # the latency: an emitted step is B .. 2 B - 1 behind the count once a block is out
            N = n_r + 5 * B + 3
            assert B <= N - lr.emitted(N, n_r, B) <= 2 * B - 1
    assert any(s % 64 for s in STARTS) and (2 ** 62 - 10 ** 6) % 64 == 0
    for bad in [(0, 0, -1, 8), (0, 0, 2 ** 31, 8), (2 ** 62 + 1, 0, 5, 8), (5, 6, 5, 8), (2 ** 62 - 2, 0, 5, 8)]:
        assert lib_steps(zfft_lib, *bad) == 0, bad


# ---------------------------------------------------------------- the model
def test_the_model_is_prefix_stable():
    x, key = lr.noise(700, 3, 1), lr.noise(700, 3, 2)
    for n_r in (0, 13, 2 ** 32 - 100, 2 ** 62 - 10 ** 6):
        for B, H in ((8, 0), (16, 5), (64, 2)):
            for k in (None, key):
                whole = lr.model_push(x, n_r, B, H, key=k, squelch=3e-4)
                assert whole.shape == (lr.steps(n_r, n_r, 700, B), 3) and whole.dtype == F32
                for n in (1, B - 1, B, 2 * B - 1, 2 * B, 2 * B + 1, 333, 699):
                    part = lr.model_push(x[:n], n_r, B, H, key=None if k is None else k[:n], squelch=3e-4)
                    assert part.shape == (lr.steps(n_r, n_r, n, B), 3) and part.tobytes() == whole[:len(part)].tobytes(), (n_r, B, H, n)


def test_the_overshoot_bound_on_adversarial_inputs():
    target = 0.5
    bound = target * (1 + 2.0 ** -21)
    rng = np.random.default_rng(4)
    worst = 0.0
    for B, H in ((8, 0), (8, 1), (16, 0), (16, 3), (64, 2)):
        n = 40 * B
        cases = []
        quiet = (1e-5 * rng.uniform(-1, 1, (n, 1))).astype(F32)
        for at in (10 * B, 11 * B - 1, 20 * B, 20 * B - 1):  # a peak on a block's first and last step
            x = quiet.copy()
            x[at] = 1.0
            cases.append(x)
        step = quiet.copy()                                # 100 dB up and down again, on and off the grid
        step[12 * B + 3:25 * B - 2] *= F32(1e5)
        cases.append(step)
        cases.append((rng.uniform(-1, 1, (n, 1)) * 10.0 ** rng.uniform(-5, 0, (n, 1))).astype(F32))   # every step another level
        cases.append(lr.noise(n, 1, 9))
        big = quiet.copy()                                 # the cap itself, and values that round against the bound
        big[15 * B] = 2.0 ** 60
        big[16 * B + 1] = np.nextafter(F32(2.0 ** 60), F32(0))
        cases.append(big)
        third = (rng.uniform(0.3, 3.0, (n, 1)) * np.where(rng.uniform(size=(n, 1)) < 0.1, 1.0, 1e-3)).astype(F32)
        cases.append(third)
        for n_r in (0, 3):
            for x in cases:
                y = lr.model_push(x, n_r, B, H, target=target, gmax=1e4, floor=1e-6)
                assert np.isfinite(y).all()
                worst = max(worst, float(np.abs(y).max()) / target)
                assert np.abs(y.astype(np.float64)).max() <= bound, (B, H, n_r, float(np.abs(y).max()))
    print(f"worst |y| / target over the cases: 1 + {worst - 1:.3e} (the bound: 1 + {2.0 ** -21:.3e})")
    assert worst > 0.999                                   # the bound is approached: the target is reached


def test_the_squelch_closes_exactly_below_its_level_and_ramps_from_and_to_zero():
    B, H, sq = 8, 1, 2.0 ** -7
    par = dict(target=0.5, gmax=1e4, floor=1e-6, squelch=sq)
    lv = F32([0.5, 0.5, np.nextafter(F32(sq), F32(0)), 0.001, sq, 0.5, 0.5, 0.001, 0.001, 0.001, 0.5, 0.5])
    key = np.repeat(lv, B)[:, None].astype(F32)
    b0, P, E, G = lr.blocks(key, 0, B, H, **par)
    assert b0 == 0 and np.array_equal(P[:, 0], lv)
    assert np.array_equal(E[:, 0], np.maximum(lv, np.concatenate([[0], lv[:-1]]).astype(F32)))
    closed = E[:, 0] < F32(sq)
    assert closed.tolist() == [False, False, False, True, False, False, False, False, True, True, False, False]
    assert (G[closed, 0] == 0).all() and (G[~closed, 0] > 0).all() and G[4, 0] == F32(64.0)              # E = squelch itself is open
    g = lr.model_push(np.ones_like(key), 0, B, H, key=key, **par)[:, 0]                                  # x = 1: the gains themselves
    assert len(g) == 11 * B
    blk = lambda b: g[b * B:(b + 1) * B]
    assert (blk(3) == 0).all() and (blk(8) == 0).all() and (blk(9) == 0).all()                          # closed on both sides: silence
    assert blk(2).tolist() == [1.0 - i / 8 for i in range(8)]                                            # to zero over block 2
    assert blk(4).tolist() == [i / 8 for i in range(8)] and blk(7).tolist() == blk(2).tolist()           # from zero over block 4
    assert blk(0)[0] == 0 and blk(1).tolist() == [1.0] * 8                                               # the start is closed: E = 0 before it
    # squelch off: the first block starts from the gain of the silence before it, limited by gmax
    y0 = lr.model_push(key, 0, B, H, target=0.5, gmax=4.0, floor=1e-6, squelch=0.0)[:, 0]
    assert y0[0] == key[0, 0] and (np.abs(y0) <= 0.5 * (1 + 2.0 ** -21)).all()


def test_the_meter_of_the_model():
    x = lr.noise(100, 2, 5)
    E, G = lr.meter(x[:7], 0, 8, 2)
    assert (E == 0).all() and (G == F32(1e4)).all()
    E, G = lr.meter(x[:17], 0, 8, 2)
    assert np.array_equal(E, np.abs(x[:16]).max(axis=0)) and np.array_equal(G, lr.gain(E, **lr.DEFAULTS))
    E, G = lr.meter(x, 0, 8, 2)
    assert np.array_equal(E, np.abs(x[72:96]).max(axis=0))


# ---------------------------------------------------------------- the chooser
def test_form_through_the_hook(zfft_lib):
    for K in (1, 2, 7, 8, 9, 64, 70, 2048):
        for B in (8, 64, 1024):
            for H in (0, 5, 73, 4096):
                n0, n_r, n = 2 ** 40 + 3 + 5 * B, 2 ** 40 + 3, 100003
                f = level_form(zfft_lib, K, B, H, n0, n_r, n)
                streams = K >= 8
                assert f["kind"] == (lr.STREAMS if streams else lr.TIME), (K, B, H)
                assert f["rows"] % B == 0 and f["rows"] >= 256 and f["piece"] == min(f["chunk"], B)
                if streams:
                    assert f["lanes"] == min(64, 1 << (K - 1).bit_length()) and f["chunk"] * (256 // f["lanes"]) == f["rows"]
                    assert f["lds_bytes"] == 4 * f["lanes"] * f["rows"] // f["piece"]
                else:
                    assert f["lanes"] == K and f["chunk"] == max(B, 64) and f["lds_bytes"] == 0
                assert f["lane_tiles"] == -(-K // f["lanes"]) and f["g_lane_tiles"] == -(-K // f["g_lanes"])
                assert f["g_lds_bytes"] == 8 * f["g_lanes"] * (f["g_blocks"] + H) <= 64 * 1024 and f["g_blocks"] >= 1
                assert f["outs"] == lr.steps(n0, n_r, n, B) and f["u_in0"] == 2 * B + n0 % B and f["u_in1"] == f["u_in0"] + n
                base = (n0 // B - 2) * B
                assert f["e0u"] == lr.emitted(n0, n_r, B) - base and f["e1u"] == lr.emitted(n0 + n, n_r, B) - base
                assert f["nq"] == (n0 + n) // B - n0 // B + 2 and f["npk"] == f["nq"] + H
                assert 1 <= f["p_grid"] <= min(f["p_tiles"], 4096) and 1 <= f["g_grid"] <= 4096 and 1 <= f["a_grid"] <= 4096
    for bad in [(0, 8, 0), (2049, 8, 0), (4, 4, 0), (4, 12, 0), (4, 2048, 0), (4, 8, -1), (4, 8, 4097), (4, 8, 0, 0, 0, 0),
                (4, 8, 0, 0, 0, 2 ** 31), (4, 8, 0, 5, 6, 5), (4, 8, 0, 2 ** 62 - 2, 0, 5)]:
        assert level_form(zfft_lib, *bad) is None, bad


def test_level_form_sweep_sanitized(tmp_path):
    """The chooser, the cut, emitted() and the ranges the kernels index over their domain as a
    stand-alone g++ program (no HIP, no Python in the child) under AddressSanitizer + UBSan:
    tests/host/level_form_sweep.cpp."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/host/level_form_sweep.cpp"
    csrc = os.path.join(ROOT, "pypanadapter_amd", "csrc")
    exe = str(tmp_path / "level_form_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", csrc, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "level_form_sweep.cpp"),
                    os.path.join(csrc, "zfft_level_plan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "level_form_sweep: ok" in r.stdout, r.stdout


# ---------------------------------------------------------------- names and errors
def test_new_names_signatures_and_errors_that_need_no_device(zfft_lib):
    from pypanadapter_amd import _lib
    import pypanadapter_amd as pkg
    declared = header_functions()
    for name in NAMES:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert getattr(zfft_lib, name).argtypes is not None and getattr(zfft_lib, name).restype is ctypes.c_int, name
    I32, I64, P, D, F = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double, ctypes.c_float
    assert zfft_lib.zfft_plan_level.argtypes == [P, I32, I32, I32, F, F, F, F]
    assert zfft_lib.zfft_level_push_device.argtypes == [P, P, I64, I64, P, I64, P, P]
    assert zfft_lib.zfft_level_push.argtypes == [P, P, P, I64, I64, P, P]
    assert zfft_lib.zfft_level_reset.argtypes == [P, I64]
    assert zfft_lib.zfft_level_meter.argtypes == [P, P, P]
    for name in ("set_level", "level_shape", "level_steps", "level_push", "level_push_device", "level_state", "level_reset",
                 "level_info", "level_meter"):
        assert callable(getattr(pkg.ZoomFFT, name)), name
    assert isinstance(pkg.LevelControl, type) and callable(pkg.LevelControl.for_demodulator) and callable(pkg.Resampler.for_level)
    # a null plan is EINVAL before anything touches a device
    v32, v64, u64, dbl, flt = I32(), I64(), ctypes.c_uint64(), D(), F()
    h = np.float32([1.0] * 24)
    hp = h.ctypes.data_as(P)
    r = ctypes.byref
    assert zfft_lib.zfft_plan_level(None, 1, 8, 0, 0.5, 1e4, 1e-6, 0.0) == EINVAL
    assert zfft_lib.zfft_level_shape(None, r(v32), r(v32), r(v32), r(flt), r(flt), r(flt), r(flt)) == EINVAL
    assert zfft_lib.zfft_level_steps(None, 5, r(v64)) == EINVAL
    assert zfft_lib.zfft_level_push_device(None, hp, 1, 1, None, 0, hp, None) == EINVAL
    assert zfft_lib.zfft_level_push(None, hp, None, 1, 1, hp, None) == EINVAL
    assert zfft_lib.zfft_level_state(None, r(u64)) == EINVAL
    assert zfft_lib.zfft_level_reset(None, 0) == EINVAL
    assert zfft_lib.zfft_level_info(None, r(dbl), r(dbl), r(dbl)) == EINVAL
    assert zfft_lib.zfft_level_meter(None, hp, hp) == EINVAL
    # the wrapper's own refusals name the value
    class _Audio:
        rate, streams, _plan = 18750.0, 4, None
    with pytest.raises(ValueError, match="hold_s = 20.0 s is 5860 blocks"):
        pkg.LevelControl.for_demodulator(_Audio, attack_s=64 / 18750.0, hold_s=20.0)
    with pytest.raises(ValueError, match="block = 48"):
        pkg.LevelControl(None, 4, 18750.0, block=48)
    with pytest.raises(ValueError, match="hold = 5000"):
        pkg.LevelControl(None, 4, 18750.0, block=64, hold=5000)
    text = open(os.path.join(ROOT, "include", "zfft.h")).read()
    rule = text[text.index("/* Level bank:"):text.index("int zfft_plan_level(")]
    for clause in ("bit for bit", "2 B - 1 unemitted steps", "(1 + 2^-21)", "(1 + 2^-24)^4", "level is off", "level_peaks",
                   "level_gains", "level_apply", "correctly rounded", "min(|v|, 2^60)", "max(n_r, B (floor(N / B) - 1))",
                   "fma(float32(i) / B, d, g_lo)", "push 2 B zeros", "H + 3 values", "squelch > 0 and E < squelch"):
        assert clause in rule, clause
