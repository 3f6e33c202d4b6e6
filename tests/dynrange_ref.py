"""Dynamic-range cases, their float32 yardstick and the gates built on it, shared by
tests/test_dynrange_host.py (CPU), tests/test_gpu_dynrange.py and tools/gen_golden.py --dynrange.

Every case is a carrier of amplitude 1.0 that the decimator must remove (or, in the transition
band, attenuate) plus weak in-band content 60 or 100 dB under it: a tone at 0.31 of the displayed
half-width plus noise (synth.make_iq; its `tones` fractions may exceed 1).

dec32: the reference's cascade -- decimate(x, 2) log2(zoom) times (pypanadapter_spectrum.py:
2096-2098), i.e. sosfiltfilt of the cheby1 sections with padlen 27 and odd extension, then [::2]
-- restated so that it runs in float32 (float32 sections and initial states, complex64 data) as
well as in float64, where it equals oracle.coracle.zoomfft.

The decimated-IQ gate, relative to the input's peak A = max |x|:

    bound(path, case) = tol(path) * S(case) + trunc(path, case)

* tol(path): the path's existing constant (path_tol, imported from the tests that own it);
* S(case) = max(1, E32(case) / E32(base)), E32(x) = max |dec32(x) - dec64(x)| / max |x|, base =
  the existing tests' input (unit noise plus a unit tone at 0.0071 fs) at the case's length and
  zoom: a path may lose accuracy on these inputs only in proportion as plain float32 arithmetic
  on the reference's own cascade does (a carrier's rms is its peak, Gaussian noise's about a third
  of it).  Never computed from a kernel; no case may have S > S_CAP;
* trunc(path, case): zero for the exact filters (paths 1-5); for the FC forms the float64
  difference on this very input between the launches' truncated models (|k| <= 768 / 512 / 256,
  composed for a chain) and the same models at |k| <= 2048, largest interior value over A.

The row gate (rows are 20 log10 PSD, so r = 10^(row / 40) is the amplitude): with
r_fs = A sum(w) / sqrt(fs sum(w^2)) the level of a bin-centred carrier of amplitude A,
|e_n| <= B A moves a segment's bin by at most 2 B A sum(w) (2: the constant detrend), by
Minkowski's inequality over the segments |r_got - r_ref| <= 2 B r_fs, and Welch's own float32
error is gated at AMP_TOL of a full-scale bin in PSD, AMP_TOL / 2 in amplitude:

    |r_got - r_ref| <= (2 bound(path, case) + AMP_TOL / 2) r_fs     for every column.

The AMP_TOL / 2 term is a flat allowance, not a measurement: the Welch stage's own share is
measured, against its own float32 yardstick, in tests/test_gpu_welch_dynrange.py
(tests/welch_dynrange_ref.py)."""
import json
import os

import numpy as np
import scipy.signal as ss

from oracle import coracle
from pypanadapter_amd import synth

FS = 2.4e6
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DELTA = 0.23                       # the image's offset from k fs / z, in displayed half-widths
LEVELS = {"p60": (1e-3, 3e-4), "p100": (1e-5, 3e-6)}   # in-band (tone amplitude, noise) under the unit carrier
# the smallest frames that reach each kernel: five FC windows and an odd tail; the shortest whose
# 1/8-rate output still takes an FC tail launch; the existing chain test's length
LENGTHS = {2: 32768 + 5, 4: 32768 + 5, 8: 32768 + 5, 16: 131072 + 5, 64: (1 << 20) + 3}
FUSED_L = 65536 + 5                # path 2 needs 8 edge windows of 8192 samples at zoom 8
S_CAP = 8.0
K_WIDE = 2048                      # the "untruncated" models' half-length
EDGE_PAD = 27                      # sosfiltfilt's padlen for four sections


# ----------------------------------------------------------------------------- the case table
def carrier_frac(kind, zoom, n_fft, n_win):
    """The carrier's frequency relative to f_lo, in displayed half-widths (synth.make_iq's unit)."""
    hw = synth.display_halfwidth_hz(1.0, n_fft, zoom, n_win)      # in units of fs
    if kind.startswith("alias"):                  # k fs / z + delta
        return int(kind[5:]) / zoom / hw + DELTA
    if kind == "neg":                             # -(2 fs / z + delta); zoom 2: -(fs / 2 + delta)
        return -(min(2, zoom // 2) / zoom / hw + DELTA)
    if kind == "trans":                           # 1.04 x the last stage's cutoff: 0.052 (8 / z) fs
        return 0.052 * 8 / zoom / hw
    if kind == "edge":                            # the first stage's passband edge, 0.19 fs
        return 0.19 / hw
    raise ValueError(kind)


def alias_ks(zoom):
    """k in {1, 2, z/4, z/2} that name an image (an integer, 1 <= k <= z/2), duplicates dropped."""
    return sorted({k for k in (1, 2, zoom // 4, zoom // 2) if 1 <= k <= zoom // 2})


def _case_table():
    cases = []

    def add(zoom, kind, level, L=None, f_lo=1.0, flip=False, tag=""):
        i = len(cases)
        tone_amp, noise = LEVELS[level]
        n_fft = 2048 if zoom == 2 else 1024
        cases.append(dict(
            name=f"z{zoom}_{kind}_{level}{tag}", zoom=zoom, kind=kind, level=level, n_fft=n_fft,
            n_win=n_fft // zoom, n_samples=LENGTHS[zoom] if L is None else L, seed=7100 + i, fs=FS,
            f_lo=f_lo, flip=flip, noise=noise,
            tones=[[carrier_frac(kind, zoom, n_fft, n_fft // zoom), 1.0], [0.31, tone_amp]]))

    lv = ("p60", "p100")
    for zoom in (8, 4, 2, 16):
        # zoom 16, k = 2: S = 8.4 > S_CAP on 131077 samples (float32's loss at that frame's ends),
        # so the case is replaced, not the cap: "neg" drives the same image from -(2 fs / z + delta)
        ks = [k for k in alias_ks(zoom) if (zoom, k) != (16, 2)]
        kinds = [f"alias{k}" for k in ks] + ["neg", "trans"] + (["edge"] if zoom >= 4 else [])
        for j, kind in enumerate(kinds):
            add(zoom, kind, lv[j % 2])
    add(8, "alias1", "p100", f_lo=150001.0, tag="_lo150k")
    add(8, "alias2", "p60", flip=True, tag="_flip")
    for j, kind in enumerate(("alias1", "trans", "edge")):       # path 2's own length
        add(8, kind, lv[j % 2], L=FUSED_L, tag="_fused")
    add(64, "alias1", "p60")
    add(64, "alias16", "p100")
    return cases


CASES = _case_table()
BY_NAME = {c["name"]: c for c in CASES}
# the cases whose rows are recorded from the reference's own update path (zoom 2, 4 and 8)
RECORDED = ["z8_alias1_p60", "z8_trans_p60", "z8_edge_p100", "z8_alias1_p100_lo150k",
            "z4_alias2_p100", "z4_trans_p100", "z2_alias1_p60", "z2_trans_p60"]
# the forced paths the decimated-IQ test runs per zoom; path 2 on the "_fused" cases alone
PATHS = {8: (1, 3, 4, 5, 6), 4: (1, 3, 4, 5, 6), 2: (1, 3, 4, 7), 16: (3, 4, 6, 7), 64: (0, 7)}


def paths_of(c):
    return (2,) if c["name"].endswith("_fused") else PATHS[c["zoom"]]


def case_input(c):
    """The frame as the plan receives it (a flip case's plan reverses it itself)."""
    return synth.make_iq(c["n_samples"], c["fs"], c["seed"], n_fft=c["n_fft"], zoom=c["zoom"],
                         n_win=c["n_win"], f_lo=c["f_lo"], tones=[tuple(t) for t in c["tones"]],
                         noise=c["noise"])


def case_signal(c, x=None):
    """The frame as the cascade sees it: reversed for a flip case."""
    x = case_input(c) if x is None else x
    return np.ascontiguousarray(x[::-1]) if c["flip"] else x


def base_input(L, seed=4400):
    """The existing *_decimate_vs_oracle tests' input: unit noise plus a unit tone at 0.0071 fs."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(L) + 1j * rng.standard_normal(L)).astype(np.complex64)
    return x + np.exp(2j * np.pi * 0.0071 * np.arange(L)).astype(np.complex64)


def fixture():
    with open(os.path.join(GOLDEN, "dynrange.json")) as fh:
        return json.load(fh)


def fixture_rows():
    return np.load(os.path.join(GOLDEN, "dynrange.npz"))


# ----------------------------------------------------------------------------- the float32 restatement
def local_oscillator(L, fs, f_lo):
    return np.sqrt(2.0) * np.exp(-2j * np.pi * np.mod(np.arange(L) * (f_lo / fs), 1.0))


def _filtfilt(sos, zi, x):
    """scipy.signal.sosfiltfilt(sos, x) (padtype 'odd', padlen 27) in x's own precision."""
    if len(x) <= EDGE_PAD:
        raise ValueError("stage input must be longer than padlen = 27")
    ext = np.concatenate([2 * x[0] - x[EDGE_PAD:0:-1], x, 2 * x[-1] - x[-2:-EDGE_PAD - 2:-1]])
    y, _ = ss.sosfilt(sos, ext, zi=zi * ext[0])
    y, _ = ss.sosfilt(sos, y[::-1], zi=zi * y[-1])
    return y[::-1][EDGE_PAD:-EDGE_PAD]


def dec32(x, zoom, fs=FS, f_lo=1.0, single=True):
    """The reference's zoomfft (mix, then decimate(., 2) log2(zoom) times) on a complex64 frame:
    single=True in float32 -- the mixed frame rounded to complex64, float32 sections -- and
    single=False in float64 (the oracle)."""
    sos, zi = coracle.decim_filter()
    y = np.asarray(x, np.complex64).astype(np.complex128) * local_oscillator(len(x), fs, f_lo)
    if single:
        sos, zi, y = sos.astype(np.float32), zi.astype(np.float32), y.astype(np.complex64)
    for _ in range(int(np.log2(zoom))):
        y = _filtfilt(sos, zi, y)[::2]
        assert y.dtype == (np.complex64 if single else np.complex128)
    return y


def e32(x, zoom, fs=FS, f_lo=1.0, d64=None):
    """max |dec32(x) - dec64(x)| / max |x|, frame ends included."""
    d64 = dec32(x, zoom, fs, f_lo, single=False) if d64 is None else d64
    return float(np.abs(dec32(x, zoom, fs, f_lo) - d64).max() / np.abs(x).max())


_BASE_E32 = {}


def base_e32(L, zoom):
    if (L, zoom) not in _BASE_E32:
        _BASE_E32[(L, zoom)] = e32(base_input(L), zoom)
    return _BASE_E32[(L, zoom)]


def s_factor(c, x=None):
    x = case_signal(c, x)
    return max(1.0, e32(x, c["zoom"], c["fs"], c["f_lo"]) / base_e32(len(x), c["zoom"]))


# ----------------------------------------------------------------------------- the truncation term
def fc_taps_k(z):
    """The K of fc_decim_kernel<z>, from where the table tests take it."""
    if z == 2:
        import test_fc2_tables
        return test_fc2_tables.K
    import test_fc_tables
    return test_fc_tables.GEO[z]["K"]


_G = {}


def g_response(z, K):
    """The z-fold model's zero-phase input-rate response |H(z)|^2 (|H(z^2)|^2 (|H(z^4)|^2)) of
    scipy's cheby1 sections on |k| <= K (the recipe of tools/fc_model.g_full, test_fc_tables._g
    and test_fc2_tables._g_full)."""
    if z not in _G:
        imp = np.zeros(6000)
        imp[0] = 1
        h = ss.sosfilt(ss.cheby1(8, 0.05, 0.4, output="sos"), imp)
        r = np.convolve(h, h[::-1])
        g = r
        for up in (2, 4)[:int(np.log2(z)) - 1]:
            ru = np.zeros((len(r) - 1) * up + 1)
            ru[::up] = r
            g = ss.fftconvolve(g, ru)
        _G[z] = g
    c = len(_G[z]) // 2
    return _G[z][c - K:c + K + 1]


def fc_model64(x, gk, z):
    """tools/fc_model.model_fp64 at a decimation of z: the zero-extended frame through the
    zero-phase FIR gk, then [::z]."""
    K = (len(gk) - 1) // 2
    return ss.fftconvolve(x, gk)[K:K + len(x)][::z]


def fc_launches(path, zoom):
    """[(z, K or None)] per launch of a forced path's schedule on one frame of the case lengths:
    K = the FC kernel's truncation, None = a launch that applies the exact filter."""
    if path == 6 and zoom in (4, 8):
        return [(zoom, fc_taps_k(zoom))]
    if path == 6 and zoom == 16:
        return [(8, fc_taps_k(8)), (2, None)]          # FC head, then zoom 2's tiles
    if path == 7 and zoom == 2:
        return [(2, fc_taps_k(2))]
    if path == 7 and zoom == 16:
        return [(8, fc_taps_k(8)), (2, fc_taps_k(2))]
    if path == 7 and zoom == 64:
        return [(8, fc_taps_k(8)), (8, fc_taps_k(8))]
    return []


def trunc_term(c, launches, x=None):
    """Largest interior |truncated models - models at K_WIDE| on the case's mixed frame, over
    A = max |x|; the interior leaves out the outputs within the wide responses' reach of an end."""
    if not launches:
        return 0.0
    x = case_signal(c, x)
    y = x.astype(np.complex128) * local_oscillator(len(x), c["fs"], c["f_lo"])
    yk, yw, rate, reach = y, y, 1, 0
    for z, K in launches:
        gw = g_response(z, K_WIDE)
        yk = fc_model64(yk, gw if K is None else g_response(z, K), z)
        yw = fc_model64(yw, gw, z)
        reach += K_WIDE * rate
        rate *= z
    m = -(-reach // rate) + 1
    assert len(yk) > 4 * m, (c["name"], len(yk), m)
    return float(np.abs(yk - yw)[m:-m].max() / np.abs(x).max())


def trunc_key(launches):
    return "+".join(f"fc{z}k{K}" if K else f"x{z}" for z, K in launches)


TRUNC_FORMS = {z: sorted({trunc_key(fc_launches(p, z)) for p in (6, 7) if fc_launches(p, z)})
               for z in (2, 4, 8, 16, 64)}


def trunc_terms(c, x=None):
    """{form: trunc} for every FC schedule the tests force at the case's zoom."""
    out = {}
    for p in (6, 7):
        ln = fc_launches(p, c["zoom"])
        if ln and trunc_key(ln) not in out:
            out[trunc_key(ln)] = trunc_term(c, ln, x)
    return out


# ----------------------------------------------------------------------------- the gates
def path_tol(path, zoom):
    """The path's existing decimated-IQ constant, from the test that owns it."""
    from test_gpu_fc import FC_TOL
    from test_gpu_fc2 import CHAIN_TOL, FC2_TOL
    from test_gpu_pc import HEAD_TOL, PC_TOL
    if path == 1:
        return 2e-6                                # include/zfft.h, zfft_plan_path
    if path == 2:
        return 3e-6                                # test_fused_interior_matches_exact_pipeline
    if path == 3:
        return 1e-5 * np.log2(zoom)                # the same test's XA bound
    if path in (0, 4, 5) or (path == 6 and zoom >= 16):
        return PC_TOL if zoom <= 8 else HEAD_TOL
    if path == 6:
        return FC_TOL
    if path == 7:
        return FC2_TOL["fc2/decimate"] if zoom == 2 else CHAIN_TOL[zoom]
    raise ValueError(path)


def iq_bound(path, c, rec):
    """bound(path, case), relative to the input's peak; rec = the case's recorded S and trunc."""
    ln = fc_launches(path, c["zoom"])
    assert rec["S"] <= S_CAP, (c["name"], rec["S"])
    return path_tol(path, c["zoom"]) * rec["S"] + (rec["trunc"][trunc_key(ln)] if ln else 0.0)


def welch_window(n_fft, n_dec, window="hamming"):
    return np.asarray(ss.get_window(window, min(n_fft, n_dec)), np.float64)


def r_fullscale(A, fs, w):
    """r = 10^(row / 40) of a bin-centred carrier of amplitude A."""
    return A * w.sum() / np.sqrt(fs * (w ** 2).sum())


def row_amp(row):
    """r = 10^(row / 40); a -inf bin gives 0."""
    return 10.0 ** (np.asarray(row, np.float64) / 40.0)


def row_gate(bound, A, fs, w, amp_tol):
    return (2.0 * bound + amp_tol / 2.0) * r_fullscale(A, fs, w)
