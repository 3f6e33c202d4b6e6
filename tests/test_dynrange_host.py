"""CPU side of the dynamic-range tests (tests/dynrange_ref.py has the cases and the gates; the
fixtures tests/golden/dynrange.json / dynrange.npz come from tools/gen_golden.py --dynrange):

* the float64 oracles reproduce the rows the reference recorded for these inputs, at
  test_oracle_golden.py's tolerances;
* dec32 in float64 mode is the oracle, so its float32 mode is the reference's own cascade in
  float32 and nothing else;
* S and the truncation terms recomputed here agree with the recorded ones, and no S exceeds 8;
* the decimated-IQ gate discriminates: numpy models of FC (tools/fc_model.py) that are wrong on
  purpose exceed it by >= 100 x on an alias case, the honest float32 model passes every zoom-8
  case's interior."""
import os
import sys

import numpy as np
import pytest

import dynrange_ref as dr
from conftest import ROOT, assert_row_close

sys.path.insert(0, os.path.join(ROOT, "tools"))
import fc_model  # noqa: E402

FIX = {c["name"]: c for c in dr.fixture()["cases"]}
Z8 = [c for c in dr.CASES if c["zoom"] == 8]
INTERIOR = 400        # outputs left out at each end (3200 input samples: tools/fc_model.main's margin)


def test_fixture_holds_the_case_table():
    from pypanadapter_amd import synth
    assert list(FIX) == [c["name"] for c in dr.CASES]
    for c in dr.CASES:
        rec = FIX[c["name"]]
        assert all(rec[k] == v for k, v in c.items()), c["name"]
        assert synth.digest(dr.case_input(c)) == rec["input_sha256"], c["name"]
        assert rec["recorded_row"] == (c["name"] in dr.RECORDED)
        assert set(rec["trunc"]) == set(dr.TRUNC_FORMS[c["zoom"]])
    assert sorted(dr.fixture_rows().files) == sorted(dr.RECORDED)
    assert {c["zoom"] for c in dr.CASES} == {2, 4, 8, 16, 64}
    assert any(c["f_lo"] == 150001.0 for c in dr.CASES) and any(c["flip"] for c in dr.CASES)


def test_case_carriers_are_where_the_issue_puts_them():
    """Relative to f_lo, in units of fs: k / z + delta, -(2 / z + delta), 0.052 (8 / z), 0.19."""
    from pypanadapter_amd import synth
    for c in dr.CASES:
        z = c["zoom"]
        hw = synth.display_halfwidth_hz(1.0, c["n_fft"], z, c["n_win"])
        f = c["tones"][0][0] * hw
        want = {"neg": -(min(2, z // 2) / z + dr.DELTA * hw), "trans": 0.052 * 8 / z, "edge": 0.19}
        if c["kind"].startswith("alias"):
            want[c["kind"]] = int(c["kind"][5:]) / z + dr.DELTA * hw
        assert abs(f - want[c["kind"]]) < 1e-12, c["name"]
        assert c["tones"][0][1] == 1.0 and c["tones"][1] == [0.31, dr.LEVELS[c["level"]][0]]
    for z in (2, 4, 8, 16):
        kinds = {c["kind"] for c in dr.CASES if c["zoom"] == z}
        assert {"neg", "trans"} <= kinds and ("edge" in kinds) == (z >= 4)
        # every image k of {1, 2, z/4, z/2}; zoom 16's k = 2 is driven by "neg" (S > 8 otherwise)
        assert {k for k in kinds if k.startswith("alias")} == \
            {f"alias{k}" for k in dr.alias_ks(z) if (z, k) != (16, 2)}
    assert dr.alias_ks(8) == [1, 2, 4] and dr.alias_ks(2) == [1] and dr.alias_ks(16) == [1, 2, 4, 8]


@pytest.mark.parametrize("name", dr.RECORDED)
def test_oracles_reproduce_the_recorded_rows(oracle_lib, name):
    from oracle import scipy_path
    c = dr.BY_NAME[name]
    x = dr.case_input(c)
    ref = dr.fixture_rows()[name]
    row = oracle_lib.psd_row(x, c["fs"], c["n_fft"], c["zoom"], c["n_win"], "hamming", c["f_lo"])
    assert_row_close(row, ref, name, db_tol=1e-8, amp_tol=1e-9)
    row = scipy_path.psd_row(x, c["fs"], c["n_fft"], c["zoom"], c["n_win"], "hamming", c["f_lo"])
    assert_row_close(row, ref, name, db_tol=1e-9, amp_tol=1e-12)


@pytest.mark.parametrize("c", dr.CASES, ids=lambda c: c["name"])
def test_dec32_in_float64_is_the_oracle_and_s_and_trunc_are_the_recorded_ones(oracle_lib, c):
    x = dr.case_signal(c)
    rec = FIX[c["name"]]
    d64 = dr.dec32(x, c["zoom"], c["fs"], c["f_lo"], single=False)
    ref = oracle_lib.zoomfft(x, c["zoom"], c["fs"], c["f_lo"])
    assert d64.shape == ref.shape
    assert np.abs(d64 - ref).max() <= 1e-12 * np.abs(ref).max()
    e = dr.e32(x, c["zoom"], c["fs"], c["f_lo"], d64)
    S = max(1.0, e / dr.base_e32(len(x), c["zoom"]))
    print(f"{c['name']}: E32 {e:.3e} S {S:.3f} (recorded {rec['S']:.3f})")
    assert abs(S - rec["S"]) <= 0.25 * rec["S"], (S, rec["S"])
    assert S <= dr.S_CAP and rec["S"] <= dr.S_CAP
    for form, t in dr.trunc_terms(c, x).items():
        # 1e-12: what two float64 FFT convolutions of a unit carrier differ by on their own
        assert abs(t - rec["trunc"][form]) <= 0.25 * rec["trunc"][form] + 1e-12, (form, t, rec["trunc"][form])


def test_truncated_responses_are_the_table_tests_responses():
    """g_response is the response test_fc_tables.py / test_fc2_tables.py and tools/fc_model.py
    build, at the K they hold for each kernel; fc_model64 at zoom 8 is fc_model.model_fp64."""
    import test_fc2_tables
    import test_fc_tables
    assert (dr.fc_taps_k(8), dr.fc_taps_k(4), dr.fc_taps_k(2)) == (768, 512, 256)
    for z in (8, 4):
        want = test_fc_tables._g(z)
        np.testing.assert_allclose(dr.g_response(z, dr.fc_taps_k(z)), want, rtol=0, atol=1e-14 * want.max())
    g2 = test_fc2_tables._g_full()
    c2 = len(g2) // 2
    np.testing.assert_allclose(dr.g_response(2, 256), g2[c2 - 256:c2 + 257], rtol=0, atol=1e-14)
    np.testing.assert_allclose(dr.g_response(8, 768), fc_model.taps(768), rtol=0, atol=1e-14)
    x = dr.case_signal(Z8[0]).astype(np.complex128)[:9000]
    a, b = dr.fc_model64(x, dr.g_response(8, 768), 8), fc_model.model_fp64(x, dr.g_response(8, 768))
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-13)


def _fc_errors(decimator):
    """{case: (interior max |got - oracle| / A) / bound(path 6, case)} over the zoom-8 cases."""
    from oracle import coracle
    out = {}
    for c in Z8:
        x = dr.case_signal(c)
        ref = coracle.zoomfft(x, 8, c["fs"], c["f_lo"])
        xm = (x.astype(np.complex128) * dr.local_oscillator(len(x), c["fs"], c["f_lo"])).astype(np.complex64)
        got = decimator(xm)
        assert got.shape == ref.shape
        err = np.abs(got - ref)[INTERIOR:-INTERIOR].max() / np.abs(x).max()
        out[c["name"]] = err / dr.iq_bound(6, c, FIX[c["name"]])
    return out


def _zero_residue(x, r):
    x = x.copy()
    x[r::8] = 0
    return x


G768 = lambda: dr.g_response(8, 768)  # noqa: E731
BROKEN = {
    # the fold without the image that holds the displayed band's upper half
    "image_left_out": lambda x: fc_model.fc_decimate(x, G768(), 8192, image_gain=[0, 1, 1, 1, 1, 1, 1, 1]),
    # the response cut at |k| <= 256 instead of 768
    "K256": lambda x: fc_model.fc_decimate(x, dr.g_response(8, 256), 8192),
    # the filter table's sign flipped on one image
    "table_sign_flipped": lambda x: fc_model.fc_decimate(x, G768(), 8192, image_gain=[1, 1, 1, 1, 1, 1, 1, -1]),
    # the kernel's form of the fold sums eight residues' DFTs: one residue left out of that sum
    "residue_left_out": lambda x: fc_model.fc_decimate(_zero_residue(x, 3), G768(), 8192),
}


@pytest.mark.parametrize("what", sorted(BROKEN))
def test_gate_rejects_a_broken_fc_model(oracle_lib, what):
    ratios = _fc_errors(BROKEN[what])
    alias = {k: v for k, v in ratios.items() if "alias" in k or "neg" in k}
    print(what, {k: float("%.3g" % v) for k, v in ratios.items()})
    assert max(alias.values()) >= 100.0, alias


def test_gate_passes_the_honest_float32_fc_model(oracle_lib):
    ratios = _fc_errors(lambda x: fc_model.fc_decimate(x, G768(), 8192))
    print({k: float("%.3g" % v) for k, v in ratios.items()})
    assert max(ratios.values()) < 1.0, ratios


def test_row_gate_arithmetic():
    """r_fs is the row amplitude of a bin-centred carrier: a unit tone at bin 37 of 1024 through
    welch's own arithmetic (hamming, constant detrend, density scaling)."""
    import scipy.signal as ss
    n, fs = 1024, dr.FS
    x = np.exp(2j * np.pi * 37 * np.arange(8 * n) / n)
    _, p = ss.welch(x, fs, window="hamming", nperseg=n, nfft=n, return_onesided=False)
    w = dr.welch_window(n, len(x))
    assert abs(dr.row_amp(20 * np.log10(p[37])) / dr.r_fullscale(1.0, fs, w) - 1.0) < 1e-9
    assert dr.row_amp(-np.inf) == 0.0
    assert dr.row_gate(1e-6, 2.0, fs, w, 1e-5) == pytest.approx((2e-6 + 5e-6) * 2.0 * dr.r_fullscale(1.0, fs, w))
