"""Welch dynamic-range cases, their float32 yardstick and the gate built on it, shared by
tests/test_welch_dynrange_host.py (CPU), tests/test_gpu_welch_dynrange.py and
tools/gen_golden.py --welch-dynrange.

Every frame is at zoom 1 (Welch sees the samples as given): a full-scale component of amplitude
A = 1 inside the band (`KINDS`), a weak tone half a bin off bin -round(0.31 N / 2) and noise, the
two 60 or 100 dB under it (dynrange_ref.LEVELS), from numpy's default_rng(seed), rounded to
complex64 (real input: float32).  Frame f of a shape holds kind f mod 6 (f mod 3 for real
input), so neighbouring frames of one launch differ in mean and carrier.

welch32: the reference's Welch -- per segment a constant detrend, the periodic window and
scipy.fft, |X|^2 / (fs sum(w^2)), then the detector over the segments (mean, median with
scipy's bias, maximum) per group of g segments -- restated so that it runs in complex64 /
float32 as well as in complex128, where it reproduces welch_average_ref.ref_row.

With r = 10^(row / 40) = sqrt(PSD) and r_fs = A sum(w) / sqrt(fs sum(w^2)), the level of a
bin-centred carrier of amplitude A,

    E32(case) = max_j |r32 - r64| / r_fs                     (every column of every line)
    gate:      |r_got - r_ref| <= 8 E32(case) r_fs           for every column.

The factor 8 is not taken from any kernel: pocketfft's twiddles are correctly rounded where the
kernels' are products of up to three float32 table entries (about 4 x on the twiddle term), and a
DFT16's radix and summation order differ from pocketfft's radix 4 / 5 passes (2 x on the rest).
E32 is recorded per case in tests/golden/welch_dynrange.json and recomputed by the host test.
No case may have 8 E32 > CAP = AMP_TOL / 8: the gate is at least 4 x tighter than the flat
AMP_TOL / 2 that dynrange_ref books for the Welch stage.

These inputs cannot run under conftest.assert_row_close: float32 arithmetic itself moves a
-100 dBc bin by more than 1e-3 dB (the error scales with the carrier, not with the bin)."""
import json
import os

import numpy as np
import scipy.fft
import scipy.signal as ss
from scipy.signal._spectral_py import _median_bias

import dynrange_ref as dr

FS = dr.FS
GOLDEN = dr.GOLDEN
A = 1.0
KINDS = ("dc", "drift", "bin", "off", "neg", "nyq")
REAL_KINDS = ("dc", "bin", "off")
LEVEL_NAMES = ("p60", "p100")
FACTOR = 8.0
CAP = 1e-5 / 8.0                   # conftest.AMP_TOL / 8
E32_AGREE = 0.25                   # fixture against recomputation: scipy builds differ in the last bit
AVERAGES = {"mean": 0, "median": 1, "max": 2}


# ----------------------------------------------------------------------------- the inputs
def weak_bin(N):
    """The weak tone sits half a bin below bin -weak_bin(N)."""
    return int(round(0.31 * N / 2))


def strong(kind, N, n, real=False):
    k0 = N // 8 + 1
    if real:
        if kind == "dc":
            return np.ones(len(n))
        return np.cos(2 * np.pi * {"bin": k0, "off": k0 + 0.37}[kind] * n / N)
    if kind == "dc":
        return np.full(len(n), np.exp(0.7j))
    cycles = {"drift": 0.02, "bin": k0, "off": k0 + 0.37, "neg": -(k0 + 0.37), "nyq": N / 2 - 0.37}[kind]
    return np.exp(2j * np.pi * cycles * n / N)


def frame(N, L, kind, level, seed, real=False):
    a_w, sigma = dr.LEVELS[level]
    rng = np.random.default_rng(seed)
    n = np.arange(L, dtype=np.float64)
    f_w = -(weak_bin(N) + 0.5) / N
    if real:
        x = A * strong(kind, N, n, True) + a_w * np.cos(2 * np.pi * f_w * n) + sigma * rng.standard_normal(L)
        return x.astype(np.float32)
    x = A * strong(kind, N, n) + a_w * np.exp(2j * np.pi * f_w * n) \
        + sigma * (rng.standard_normal(L) + 1j * rng.standard_normal(L))
    return x.astype(np.complex64)


# ----------------------------------------------------------------------------- the shapes
def _shape_table():
    """One entry per GPU test: the smallest shapes that reach each Welch form.  `form` is what
    zfft__welch_plan must say of it ((fft, out, select); test_welch_dynrange_host pins it)."""
    shapes = []

    def add(tag, form, N, W, L, F, welch=0, average="mean", g=0, window="hamming", real=False, kinds=None):
        i = len(shapes)
        kinds = tuple(kinds) if kinds else (REAL_KINDS if real else KINDS)
        shapes.append(dict(
            name=f"{form[0]}_{form[1]}_{form[2]}-{tag}", form=form, n_fft=N, n_win=W, n_samples=L, frames=F,
            welch=welch, average=average, g=g, window=window, real=real, seed=9100 + 16 * i,
            kinds=[kinds[f % len(kinds)] for f in range(F)],
            levels=[LEVEL_NAMES[(i + f) % 2] for f in range(F)]))

    row, segs = "row", "segs"
    # Stockham (welch_rows_kernel): every first-pass radix (2, 4, 8, 16, 2), one and two passes
    for N in (32, 64, 128, 256, 512):
        add(f"n{N}", ("stockham", row, "none"), N, N, 3 * N, 6)
    add("n512_w300", ("stockham", row, "none"), 512, 300, 1536, 6)
    add("n512_w97", ("stockham", row, "none"), 512, 97, 1536, 6)
    # the short-input branch: nperseg = L < n_fft, zero-padded
    add("n1024_short1019", ("stockham", row, "none"), 1024, 1024, 1019, 2)
    add("n1024_short515", ("stockham", row, "none"), 1024, 1024, 515, 2)
    add("n16384_short16379", ("stockham", row, "none"), 16384, 16384, 16379, 2)
    # DIF (welch_dif_kernel<N, PRUNE, HALF = true>), row form: full and PRUNE (n_win <= 2 N / RL;
    # N = 8192 is always pruned two-sided).  HALF = false is unreachable: the DIF kernel is chosen
    # only when nperseg == n_fft, whose step is n_fft / 2, so no case is invented for it.
    for N, Ws in ((1024, (1024, 512)), (2048, (2048, 512)), (4096, (4096, 512)), (8192, (8192, 1000)),
                  (16384, (16384, 8192))):
        for W in Ws:
            add(f"n{N}_w{W}", ("dif", row, "none"), N, W, 2 * N, 2 if N == 16384 else 6)
    # the split form: per-part sums, then welch_parts_kernel (one frame of 9 segments)
    for N in (1024, 4096):
        for W in (N, 512):
            add(f"n{N}_w{W}", ("dif", "parts", "none"), N, W, 5 * N, 1)
    # four-step (welch4_*): N1 = 16, 64 forced, 128, 256 automatic; W = N detrends after the
    # transform (fused_mean); the pruned row pass needs n_win 8 <= n_fft and N1 > 16
    for N, welch in ((4096, 2), (16384, 2), (32768, 0), (65536, 0)):
        add(f"n{N}_full", ("four", row, "none"), N, N, 3 * N, 6, welch=welch)
        if N > 4096:
            add(f"n{N}_pruned", ("four", row, "none"), N, N // 8, 3 * N, 2, welch=welch)
            add(f"n{N}_w{N // 8 + 4}", ("four", row, "none"), N, N // 8 + 4, 3 * N, 2, welch=welch)
    add("n4096_means_l4089", ("four", row, "none"), 4096, 4096, 4089, 2, welch=2)
    # detectors (SEG forms, welch_select): the strong component is in every segment
    for N, fft, welch in ((512, "stockham", 0), (1024, "dif", 0), (4096, "four", 2)):
        for average in ("median", "max"):
            add(f"n{N}_{average}", (fft, segs, "reg16"), N, N, 5 * N, 3, welch=welch, average=average)
    for N, average in ((64, "median"), (128, "max"), (256, "median")):          # SEG per first radix
        add(f"n{N}_{average}", ("stockham", segs, "reg16"), N, N, 5 * N, 3, average=average)
    add("n4096_w512_max", ("dif", segs, "reg16"), 4096, 512, 5 * 4096, 3, average="max")
    for N, welch, W, average in ((16384, 2, 16384, "median"), (16384, 2, 2048, "max"), (32768, 0, 32768, "max"),
                                 (32768, 0, 4096, "median"), (65536, 0, 8192, "max")):
        add(f"n{N}_w{W}_{average}", ("four", segs, "reg8"), N, W, 3 * N, 2, welch=welch, average=average)
    # lines: fused in the DIF kernel, through the scratch behind the Stockham kernel, and the median's
    for g in (1, 2):
        add(f"n1024_g{g}", ("dif", "lines", "none"), 1024, 1024, 5 * 1024, 3, g=g)
        add(f"n512_g{g}", ("stockham", segs, "mean_lines"), 512, 512, 5 * 512, 3, g=g)
    add("n1024_g2_median", ("dif", segs, "reg4"), 1024, 1024, 5 * 1024, 3, g=2, average="median")
    # windows of 92 to 110 dB: the float32 window table against an off-bin carrier's sidelobes
    for tag, window in (("bh", "blackmanharris"), ("nuttall", "nuttall"), ("cheb100", ("chebwin", 100)),
                        ("kaiser14", ("kaiser", 14))):
        add(f"n512_{tag}", ("stockham", row, "none"), 512, 512, 1536, 2, window=window, kinds=("off", "dc"))
        add(f"n4096_{tag}", ("dif", row, "none"), 4096, 4096, 8192, 2, window=window, kinds=("off", "dc"))
        add(f"n32768_pruned_{tag}", ("four", row, "none"), 32768, 4096, 98304, 2, window=window,
            kinds=("off", "dc"))
    # real input: one-sided rows, doubled bins (three frames of five segments: the DIF kernel splits)
    add("n1024_real", ("dif", "parts", "none"), 1024, 1024, 3072, 3, real=True)
    add("n256_real", ("stockham", row, "none"), 256, 256, 768, 3, real=True)
    # (appended, so that the seeds above stay: the short-input branch at 512 threads per frame)
    add("n8192_short8189", ("stockham", row, "none"), 8192, 8192, 8189, 2)
    return shapes


SHAPES = _shape_table()
BY_NAME = {s["name"]: s for s in SHAPES}


def shape_frames(s):
    return np.stack([frame(s["n_fft"], s["n_samples"], s["kinds"][f], s["levels"][f], s["seed"] + f, s["real"])
                     for f in range(s["frames"])])


def case_name(s, f):
    return f"{s['name']}/f{f}_{s['kinds'][f]}_{s['levels'][f]}"


def plan_key(s, lines_route=0, cap_bytes=0):
    """The arguments of test_welch_plan.welch_plan for the shape's call."""
    return (s["n_fft"], s["n_win"], 1, 3 if s["real"] else 0, s["welch"], AVERAGES[s["average"]], s["g"],
            lines_route, cap_bytes, s["n_samples"], s["frames"])


def fixture():
    with open(os.path.join(GOLDEN, "welch_dynrange.json")) as fh:
        return json.load(fh)


# ----------------------------------------------------------------------------- the float32 restatement
def welch32(x, n_fft, window="hamming", average="mean", g=0, single=True, fs=FS):
    """(R, bins) densities of one frame, R = the lines of groups of g segments (g = 0: one), bins
    = n_fft two-sided in FFT order, n_fft / 2 + 1 one-sided for real x: scipy.signal's
    _spectral_helper step by step in complex64 / float32 (single) or complex128 / float64."""
    x = np.asarray(x)
    real = not np.iscomplexobj(x)
    ft, ct = (np.float32, np.complex64) if single else (np.float64, np.complex128)
    x = x.astype(ft if real else ct)
    nper = min(n_fft, len(x))
    step = nper - nper // 2
    w = ss.get_window(window, nper).astype(ft)
    nseg = (len(x) - nper) // step + 1
    seg = np.lib.stride_tricks.sliding_window_view(x, nper)[::step][:nseg]
    seg = seg - seg.mean(axis=-1, keepdims=True)
    seg = w * seg
    assert seg.dtype == (ft if real else ct)
    X = scipy.fft.rfft(seg, n=n_fft) if real else scipy.fft.fft(seg, n=n_fft)
    assert X.dtype == ct, X.dtype
    P = np.conjugate(X) * X
    P *= ft(1.0) / (ft(fs) * (w * w).sum())
    if real:
        P[..., 1:-1] *= 2
    P = P.real
    assert P.dtype == ft and w.dtype == ft, (P.dtype, w.dtype)
    G = nseg if g <= 0 or g >= nseg else g
    out = []
    for s0 in range(0, nseg, G):
        S = P[s0:s0 + G]
        if average == "mean":
            out.append(S.mean(axis=0))
        elif average == "median":
            out.append(np.median(S, axis=0) / ft(_median_bias(len(S))))
        elif average == "max":
            out.append(S.max(axis=0))
        else:
            raise ValueError(average)
        assert out[-1].dtype == ft
    return np.stack(out)


def crop(P, n_fft, n_win):
    """The reference's fftshift and slice on the last axis (one-sided rows come out shorter)."""
    P = np.fft.fftshift(P, axes=-1)
    return P[..., n_fft // 2 - n_win // 2: n_fft // 2 + n_win // 2]


def amp_lines(P, n_fft, n_win):
    """r = sqrt(PSD) of the cropped lines, float64."""
    return np.sqrt(np.abs(crop(P, n_fft, n_win)).astype(np.float64))


def r_fullscale(n_fft, n_samples, window="hamming", fs=FS):
    return dr.r_fullscale(A, fs, np.asarray(ss.get_window(window, min(n_fft, n_samples)), np.float64))


def e32(x, n_fft, n_win, window="hamming", average="mean", g=0, fs=FS):
    """max over every line and column of |r32 - r64| / r_fs."""
    r32 = amp_lines(welch32(x, n_fft, window, average, g, True, fs), n_fft, n_win)
    r64 = amp_lines(welch32(x, n_fft, window, average, g, False, fs), n_fft, n_win)
    return float(np.abs(r32 - r64).max() / r_fullscale(n_fft, len(x), window, fs))


def shape_e32(s, x=None):
    x = shape_frames(s) if x is None else x
    return [e32(x[f], s["n_fft"], s["n_win"], window_of(s), s["average"], s["g"]) for f in range(s["frames"])]


def window_of(s):
    return tuple(s["window"]) if isinstance(s["window"], (list, tuple)) else s["window"]


def gate(E32):
    """The gate in units of r_fs."""
    assert FACTOR * E32 <= CAP, E32
    return FACTOR * E32


def tone_columns(n_fft, n_win, real=False):
    """The row's columns nearest the weak tone (half a bin off: the bin on either side)."""
    bins = n_fft // 2 + 1 if real else n_fft
    cols = crop(np.arange(bins), n_fft, n_win)
    k = weak_bin(n_fft)
    want = (k, k + 1) if real else (n_fft - k, n_fft - k - 1)
    return [int(j) for j in np.flatnonzero(np.isin(cols, want))]


# ----------------------------------------------------------------------------- float32 models of the kernels
# What the forms' own float32 arithmetic gives where it differs from welch32's: the figures
# quoted in test_gpu_welch_dynrange.LIMITS (test_welch_dynrange_host recomputes them).
def model_rows32(x, n_fft, n_win, window="hamming", average="mean", g=0, fs=FS):
    """welch32's float32 densities through a float32 20 log10, the format of a row: max over the
    columns of |10^(row32 / 40) - r64| / r_fs."""
    P32 = crop(welch32(x, n_fft, window, average, g, True, fs), n_fft, n_win)
    row32 = np.float32(20.0) * np.log10(P32)
    assert row32.dtype == np.float32
    r64 = amp_lines(welch32(x, n_fft, window, average, g, False, fs), n_fft, n_win)
    return float(np.abs(dr.row_amp(row32) - r64).max() / r_fullscale(n_fft, len(x), window, fs))


def four_step32(xw, n_fft, product_twiddles=True):
    """(nseg, n_fft) complex64 -> its FFT by the four-step factorisation n = n1 + N1 n2,
    k = k2 + 256 k1 in complex64: length-256 transforms over n2, the twiddle W_N^(n1 k2), length-N1
    transforms over n1.  product_twiddles: the kernel's recipe for k2 = t + 16 i, W^(n1 t) b^i with
    b = W^(16 n1) and b^i from b^2, b^4, b^8 by squaring (zfft_fft.h, apply_powers); otherwise
    every twiddle rounded once."""
    c64 = np.complex64
    N1 = n_fft // 256
    tw = np.exp(-2j * np.pi * np.arange(n_fft) / n_fft).astype(c64)
    C = scipy.fft.fft(xw.reshape(len(xw), 256, N1), axis=1)            # [s, k2, n1]
    n1 = np.arange(N1)
    if product_twiddles:
        b = tw[16 * n1]
        b2 = b * b
        b4 = b2 * b2
        b8 = b4 * b4
        w3, w5, w6 = b * b2, b * b4, b2 * b4
        w7 = w3 * b4
        pw = [None, b, b2, w3, b4, w5, w6, w7, b8, b * b8, b2 * b8, w3 * b8, b4 * b8, w5 * b8, w6 * b8, w7 * b8]
        for t in range(16):
            a = tw[n1 * t]
            for i in range(16):
                v = C[:, t + 16 * i, :] * a
                C[:, t + 16 * i, :] = v if i == 0 else v * pw[i]
    else:
        C = C * np.exp(-2j * np.pi * (np.arange(256)[:, None] * n1[None, :]) / n_fft).astype(c64)
    X = scipy.fft.fft(C, axis=2)                                       # [s, k2, k1]
    assert C.dtype == c64 and X.dtype == c64
    return X.transpose(0, 2, 1).reshape(len(xw), n_fft)


def model_four_step(x, n_fft, n_win, average="mean", product_twiddles=True, fs=FS):
    """The four-step form with nperseg == n_fft in complex64 numpy (Hamming, g = 0): four_step32 of
    the windowed segments, the mean taken off after the transform, X = FFT(x w) - mean FFT(w) with
    FFT(w) from float64 rounded once.  Returns (max |r - r64| / r_fs, the bin where)."""
    x = np.asarray(x, np.complex64)
    step = n_fft // 2
    nseg = (len(x) - n_fft) // step + 1
    w64 = ss.get_window("hamming", n_fft)
    seg = np.lib.stride_tricks.sliding_window_view(x, n_fft)[::step][:nseg]
    mean = seg.mean(axis=-1, keepdims=True)
    X = four_step32(np.ascontiguousarray(seg * w64.astype(np.float32)), n_fft, product_twiddles) \
        - mean * scipy.fft.fft(w64).astype(np.complex64)
    assert X.dtype == np.complex64
    P = (X.real ** 2 + X.imag ** 2) * np.float32(1.0 / (fs * (w64 ** 2).sum()))
    P = {"mean": lambda: P.mean(axis=0), "median": lambda: np.median(P, axis=0) / np.float32(_median_bias(nseg)),
         "max": lambda: P.max(axis=0)}[average]()
    d = np.abs(amp_lines(P[None], n_fft, n_win) - amp_lines(welch32(x, n_fft, "hamming", average, 0, False, fs),
                                                           n_fft, n_win))[0] / r_fullscale(n_fft, len(x), "hamming", fs)
    k = int(crop(np.arange(n_fft), n_fft, n_win)[d.argmax()])
    return float(d.max()), k - n_fft if k > n_fft // 2 else k


def model_stockham_mean(x, n_fft):
    """welch_rows_kernel's mean of a full segment in complex64: thread t adds x[t + (n_fft / 16) i],
    i = 0 .. 15, in turn, then the wave's xor butterfly (n_fft <= 1024: one wave).  Returns the
    largest |mean32 - mean64| over the segments: the bin-0 error in units of r_fs for A = 1."""
    x = np.asarray(x, np.complex64)
    T16, step = n_fft // 16, n_fft // 2
    assert T16 <= 64
    worst, lane = 0.0, np.arange(64)
    for s0 in range(0, len(x) - n_fft + 1, step):
        seg = x[s0:s0 + n_fft]
        v = np.zeros(64, np.complex64)
        for i in range(16):
            v[:T16] = v[:T16] + seg[i * T16:(i + 1) * T16]
        for m in (32, 16, 8, 4, 2, 1):
            v = v + v[lane ^ m]
        worst = max(worst, abs(np.complex128(v[0] * np.float32(1.0 / n_fft)) - seg.astype(np.complex128).mean()))
    return float(worst)
