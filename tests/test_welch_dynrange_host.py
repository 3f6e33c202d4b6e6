"""CPU checks of the Welch dynamic-range yardstick (tests/welch_dynrange_ref.py): the float32
restatement welch32 tied to the float64 reference (welch_average_ref / welch_lines_ref, and
scipy.signal.welch itself for the mean), E32 against the recorded fixture, the cap on the gate,
and -- through the device-free chooser hook -- that every shape of the GPU test reaches the
Welch form its id names."""
import numpy as np
import pytest
import scipy.signal as ss

import welch_dynrange_ref as wd
import welch_lines_ref as wlr
from conftest import AMP_TOL
from test_welch_plan import welch_plan

FIX = {s["name"]: s for s in wd.fixture()["shapes"]}
_X = {}


def _frames(s):
    if s["name"] not in _X:
        _X[s["name"]] = wd.shape_frames(s)
    return _X[s["name"]]


def test_case_names_unique_and_recorded():
    names = [wd.case_name(s, f) for s in wd.SHAPES for f in range(s["frames"])]
    assert len(names) == len(set(names))
    assert len({s["name"] for s in wd.SHAPES}) == len(wd.SHAPES)
    assert sorted(FIX) == sorted(s["name"] for s in wd.SHAPES)
    for s in wd.SHAPES:
        rec = FIX[s["name"]]
        assert rec["seed"] == s["seed"]
        assert rec["cases"] == [wd.case_name(s, f) for f in range(s["frames"])]
        assert len(rec["E32"]) == s["frames"]


def test_inputs_are_single_precision_and_full_scale():
    for s in wd.SHAPES:
        x = _frames(s)
        assert x.dtype == (np.float32 if s["real"] else np.complex64)
        assert x.shape == (s["frames"], s["n_samples"])
        assert 1.0 - 2e-3 <= np.abs(x).max(axis=1).min() and np.abs(x).max() <= 1.0 + 4e-3


@pytest.mark.parametrize("s", wd.SHAPES, ids=lambda s: s["name"])
def test_welch32_in_double_is_the_reference(s):
    """welch32(single=False) against welch_lines_ref.ref_lines (g = 0: welch_average_ref.ref_row's
    row), per bin to 1e-12 relative in the density."""
    N, W = s["n_fft"], s["n_win"]
    for f, x in enumerate(_frames(s)):
        P = wd.crop(wd.welch32(x, N, wd.window_of(s), s["average"], s["g"], single=False), N, W)
        ref = wlr.ref_lines(x, wd.FS, N, 1, W, s["g"], s["average"], wd.window_of(s))
        assert P.shape == ref.shape, (P.shape, ref.shape)
        np.testing.assert_allclose(20.0 * np.log10(P), ref, rtol=0, atol=20 / np.log(10) * 1e-12,
                                   err_msg=wd.case_name(s, f))


def test_welch32_in_double_is_scipy_welch():
    for s in wd.SHAPES:
        if s["average"] != "mean" or s["g"]:
            continue
        N = s["n_fft"]
        x = _frames(s)[0].astype(np.float64 if s["real"] else np.complex128)
        nper = min(N, len(x))
        _, P = ss.welch(x, wd.FS, window=wd.window_of(s), nperseg=nper, noverlap=nper // 2, nfft=N,
                        return_onesided=s["real"], detrend="constant", scaling="density")
        np.testing.assert_allclose(wd.welch32(x, N, wd.window_of(s), single=False)[0], P, rtol=1e-12, atol=0,
                                   err_msg=s["name"])


@pytest.mark.parametrize("s", wd.SHAPES, ids=lambda s: s["name"])
def test_e32_agrees_with_the_fixture_and_the_cap_holds(s):
    assert wd.CAP == AMP_TOL / 8
    E = wd.shape_e32(s, _frames(s))
    for f, (e, rec) in enumerate(zip(E, FIX[s["name"]]["E32"])):
        assert abs(e - rec) <= wd.E32_AGREE * rec, (wd.case_name(s, f), e, rec)
        assert wd.FACTOR * rec <= wd.CAP and wd.FACTOR * e <= wd.CAP, (wd.case_name(s, f), e, rec)
        assert rec > 0


def test_every_shape_reaches_the_form_its_id_names():
    """zfft__welch_plan on every GPU shape: fft, out and select are the words of the shape's name,
    so the matrix cannot collapse onto one kernel if the chooser changes."""
    wrong = []
    for s in wd.SHAPES:
        rc, desc = welch_plan(*wd.plan_key(s))
        p = desc.split()
        got = (p[0], p[1], p[-1].split("=")[1]) if rc == 0 else (rc, desc)
        if got != tuple(s["form"]) or not s["name"].startswith("_".join(s["form"]) + "-"):
            wrong.append((s["name"], got))
        if s["form"][1] == "parts":
            assert "split=1 " not in desc, (s["name"], desc)
    assert not wrong, wrong
    forms = {tuple(s["form"]) for s in wd.SHAPES}
    assert {f[0] for f in forms} == {"stockham", "dif", "four"}
    assert {f[1] for f in forms} == {"row", "parts", "segs", "lines"}
    assert {"reg4", "reg8", "reg16", "mean_lines", "none"} <= {f[2] for f in forms}


def test_frames_of_a_launch_differ_in_kind():
    for s in wd.SHAPES:
        if s["frames"] > 1:
            assert all(a != b for a, b in zip(s["kinds"], s["kinds"][1:])), s["name"]
        assert set(s["kinds"]) <= set(wd.REAL_KINDS if s["real"] else wd.KINDS)
    assert any(s["frames"] == 6 and tuple(s["kinds"]) == wd.KINDS for s in wd.SHAPES)


def test_limits_quote_the_models():
    """Every entry of test_gpu_welch_dynrange.LIMITS names a case of the table, quotes that case's
    gate, and its "model" figure is what the float32 model of its cause gives here (within 25 %:
    scipy builds differ in the last bit)."""
    import re
    from test_gpu_welch_dynrange import LIMITS
    cases = {wd.case_name(s, f): (s, f) for s in wd.SHAPES for f in range(s["frames"])}
    assert set(LIMITS) <= set(cases)
    for name, text in LIMITS.items():
        s, f = cases[name]
        cause = text.split(":")[0]
        measured, gate, model = (float(v) for v in
                                 re.match(r"\w+: (\S+) > (\S+) at bin .*?; model ([0-9.e-]+)", text).groups())
        assert measured > gate and abs(gate - wd.gate(FIX[s["name"]]["E32"][f])) <= 0.01 * gate, name
        x = _frames(s)[f]
        N, W = s["n_fft"], s["n_win"]
        if cause == "rows":
            got = wd.model_rows32(x, N, W, wd.window_of(s), s["average"], s["g"])
        elif cause in ("detrend", "twiddles"):
            assert s["form"][0] == "four" and s["n_samples"] >= N and s["window"] == "hamming" and not s["g"]
            got, where = wd.model_four_step(x, N, W, s["average"], product_twiddles=cause == "twiddles")
            if cause == "detrend":
                assert where in (-1, 0, 1), (name, where)
            else:
                once = float(re.search(r"rounded once ([0-9.e-]+)", text).group(1))
                got_once, _ = wd.model_four_step(x, N, W, s["average"], product_twiddles=False)
                assert abs(got_once - once) <= 0.25 * once and got_once < gate < got, (name, got_once, gate, got)
                assert where % 256 == 255 and f" at bin {where};" in text, (name, where)
        else:
            assert cause == "mean" and s["form"][0] == "stockham" and s["n_samples"] >= N
            got = wd.model_stockham_mean(x, N)
        assert abs(got - model) <= 0.25 * model, (name, cause, got, model)
