"""GPU dynamic range of the Welch stage: a full-scale component inside the band -- a DC offset, a
carrier on or off a bin, at either sign and beside the fftshift seam -- with content 60 or 100 dB
under it, on every Welch FFT form (tests/welch_dynrange_ref.py has the cases, the float32
yardstick E32 and the gate; tests/golden/welch_dynrange.json the recorded E32).  Every other
Welch test feeds unit noise plus a few tones, rows that span 30 to 40 dB: whatever a kernel gets
wrong 60 dB or more under its strongest bin -- a twiddle built from table products, a mean from
the wrong slot, the four-step form's detrend after the transform, the float32 window table, the
pruned last stages' indices -- sits under that input's own noise.

    |r_got - r_ref| <= 8 E32(case) r_fs     for every column,    r = 10^(row / 40)

against the float64 reference per detector (welch_average_ref / welch_lines_ref).  These inputs
cannot run under conftest.assert_row_close: float32 arithmetic itself moves a -100 dBc bin by
more than 1e-3 dB (the error scales with the carrier).

Also here: the non-finite contract of include/zfft.h (a zero bin gives -inf, a NaN in any segment
NaN) with the neighbouring frames bytewise untouched, and the rows' exact scaling with the input
(no absolute epsilon, clamp or denormal flush in a Welch kernel)."""
import numpy as np
import pytest

import dynrange_ref as dr
import welch_average_ref as war
import welch_dynrange_ref as wd
import welch_lines_ref as wlr
from conftest import check_rel
from welch_plan_check import assert_plan_ran

pytestmark = pytest.mark.gpu
FS = wd.FS
MODES = ("mean", "median", "max")
FIX = {s["name"]: s for s in wd.fixture()["shapes"]}

# Where the kernels sit (MI355X, |r_got - r_ref| / r_fs, 229 cases): between 2e-9 and 7.4e-7 (-123 dBc),
# 205 cases inside their gate.  The 24 that miss it do so by what float32 gives, each for one of
# four causes, with the measured value, the gate, where in the row, and a float32 numpy model of
# that arithmetic (stated in include/zfft.h at zfft_plan_welch):
# * rows: the miss is at the carrier's own bin (or its main-lobe neighbour).  A row is float32 dB,
#   20.f * log10f(v): one unit in the last place of a row near -70 dB is 7.6e-6 dB = 4.4e-7 of that
#   bin's amplitude.  Model: welch32's float32 densities through numpy's float32 20 log10 (in 9 of
#   the 19 the kernel's row error is that model's to three digits), and the same bound with log10f
#   at its 2 ulp.  E32 compares densities and never sees the row format;
# * detrend: the four-step form with nperseg == n_fft takes the mean off after the transform,
#   X = FFT(x w) - mean FFT(w): two full-scale float32 quantities cancel at bins 0 and +-1, and half
#   a unit in the last place of either is up to 6e-8 of a full-scale bin per component, whatever
#   the order of the sums.  Model: that expression in complex64 numpy through the form's N1 x 256
#   factorisation, twiddles rounded once; it draws 8.2e-9 ... 7.8e-8 on the three cases where the
#   kernel draws 3.3e-8 ... 9.3e-8;
# * twiddles: the four-step form's W_N^(n1 k2) = W^(n1 t) b^i, b^i from b^2, b^4, b^8 by repeated
#   squaring, carries up to 15 x the table's rounding at k2 = 255, where a Hamming-windowed DC term
#   has 0.43 of its amplitude before the row pass cancels it.  Model: the same factorisation in
#   complex64 numpy with that recipe, and with twiddles rounded once;
# * mean: the Stockham kernel's float32 mean (16 values per thread, then the wave's butterfly)
#   against numpy's pairwise sum, on a drifting carrier.  Model: that order in complex64 numpy.
LIMITS = {
    "dif_lines_none-n1024_g2/f2_bin_p60":
        "rows: 4.23e-07 > 3.69e-07 at bin 129 (1.00 r_fs); model 3.09e-07, log10f at 2 ulp 7.69e-07",
    "dif_parts_none-n1024_real/f1_bin_p60":
        "rows: 2.34e-07 > 1.04e-07 at bin 129 (0.71 r_fs); model 2.34e-07, log10f at 2 ulp 5.43e-07",
    "dif_parts_none-n1024_real/f2_off_p100":
        "rows: 9.73e-08 > 9.30e-08 at bin 129 (0.63 r_fs); model 4.29e-07, log10f at 2 ulp 6.74e-07",
    "dif_row_none-n1024_w1024/f4_neg_p60":
        "rows: 2.52e-07 > 1.66e-07 at bin -130 (0.72 r_fs); model 2.52e-07, log10f at 2 ulp 6.89e-07",
    "dif_row_none-n2048_w2048/f2_bin_p60":
        "rows: 2.41e-07 > 2.30e-07 at bin 256 (0.43 r_fs); model 1.34e-07, log10f at 2 ulp 7.69e-07",
    "dif_row_none-n8192_w8192/f3_off_p100":
        "rows: 4.56e-07 > 4.15e-07 at bin 1025 (0.90 r_fs); model 7.82e-08, log10f at 2 ulp 5.90e-07",
    "dif_segs_reg16-n1024_max/f2_bin_p60":
        "rows: 2.88e-07 > 1.95e-07 at bin 129 (1.00 r_fs); model 2.04e-07, log10f at 2 ulp 7.69e-07",
    "four_row_none-n16384_pruned/f0_dc_p60":
        "detrend: 3.28e-08 > 2.74e-08 at bin 0; model 8.20e-09",
    "four_row_none-n65536_w8196/f1_drift_p60":
        "detrend: 6.04e-08 > 2.32e-08 at bin -1; model 7.82e-08",
    "four_segs_reg16-n4096_max/f2_bin_p60":
        "rows: 4.27e-07 > 2.77e-07 at bin 513 (1.00 r_fs); model 2.08e-07, log10f at 2 ulp 6.59e-07",
    "four_segs_reg16-n4096_median/f0_dc_p100":
        "twiddles: 7.16e-08 > 4.48e-08 at bin 767; model 6.71e-08, with twiddles rounded once 2.71e-08",
    "four_segs_reg8-n32768_w4096_median/f0_dc_p60":
        "detrend: 9.33e-08 > 3.03e-08 at bin 0; model 6.70e-08",
    "stockham_row_none-n128/f2_bin_p60":
        "rows: 4.66e-07 > 3.00e-07 at bin 17 (1.00 r_fs); model 2.06e-07, log10f at 2 ulp 1.32e-06",
    "stockham_row_none-n256_real/f2_off_p60":
        "rows: 2.55e-07 > 1.22e-07 at bin 33 (0.63 r_fs); model 2.55e-07, log10f at 2 ulp 8.35e-07",
    "stockham_row_none-n32/f3_off_p100":
        "rows: 3.70e-07 > 2.59e-07 at bin 5 (0.90 r_fs); model 3.70e-07, log10f at 2 ulp 1.18e-06",
    "stockham_row_none-n512/f2_bin_p60":
        "rows: 3.19e-07 > 2.26e-07 at bin 65 (1.00 r_fs); model 3.19e-07, log10f at 2 ulp 7.69e-07",
    "stockham_row_none-n512/f5_nyq_p100":
        "rows: 1.90e-07 > 1.15e-07 at bin 256 (0.90 r_fs); model 1.90e-07, log10f at 2 ulp 9.53e-07",
    "stockham_row_none-n512_bh/f0_off_p100":
        "rows: 5.52e-07 > 3.36e-07 at bin 65 (0.95 r_fs); model 5.52e-07, log10f at 2 ulp 1.25e-06",
    "stockham_row_none-n512_w300/f1_drift_p60":
        "mean: 1.91e-08 > 1.71e-08 at bin 0; model 4.01e-08",
    "stockham_row_none-n512_w300/f3_off_p60":
        "rows: 3.92e-07 > 1.63e-07 at bin 65 (0.90 r_fs); model 4.82e-07, log10f at 2 ulp 9.53e-07",
    "stockham_row_none-n512_w300/f4_neg_p100":
        "rows: 3.56e-07 > 1.77e-07 at bin -65 (0.90 r_fs); model 3.56e-07, log10f at 2 ulp 9.53e-07",
    "stockham_row_none-n64/f3_off_p60":
        "rows: 4.25e-07 > 3.29e-07 at bin 9 (0.90 r_fs); model 4.25e-07, log10f at 2 ulp 1.18e-06",
    "stockham_segs_reg16-n128_max/f2_bin_p60":
        "rows: 5.75e-07 > 3.22e-07 at bin 17 (1.00 r_fs); model 3.53e-07, log10f at 2 ulp 1.32e-06",
    "stockham_segs_reg16-n256_median/f2_bin_p100":
        "rows: 2.04e-07 > 2.00e-07 at bin 34 (0.49 r_fs); model 5.07e-07, log10f at 2 ulp 8.90e-07",
}


class GateMiss(Exception):
    """Exactly the cases of a shape that LIMITS lists missed the gate (strict xfail takes this alone)."""


@pytest.fixture(scope="module", autouse=True)
def _gpu(zfft_lib):
    from pypanadapter_amd import device_count
    assert device_count() >= 1, "GPU tests need a HIP device"


def _plan(s, **kw):
    from pypanadapter_amd import ZoomFFT
    plan = ZoomFFT(s["n_fft"], 1, FS, n_win=s["n_win"], window=wd.window_of(s) if "window" in s else "hamming",
                   in_dtype="f32" if s.get("real") else "complex64", **kw)
    if s.get("welch"):
        plan.set_welch(s["welch"])
    plan.set_timing(True)
    return plan


def _form(desc):
    p = desc.split()
    return p[0], p[1], p[-1].split("=")[1]


def _limited(s):
    return sorted(c for c in LIMITS if c.split("/")[0] == s["name"])


PARAMS = [pytest.param(s, id=s["name"],
                       marks=[pytest.mark.xfail(strict=True, raises=GateMiss,
                                                reason="; ".join(f"{c}: {LIMITS[c]}" for c in _limited(s)))]
                       if _limited(s) else []) for s in wd.SHAPES]


@pytest.mark.parametrize("s", PARAMS)
def test_welch_dynrange_rows_vs_float64_reference(s):
    """One plan at zoom 1, one call on the shape's frames (frame f holds kind f mod 6), the form
    that ran confirmed, then every column of every frame's row (or lines) against the gate.  A
    shape with cases in LIMITS is an expected failure only while exactly those cases miss."""
    N, W, L, F, g = s["n_fft"], s["n_win"], s["n_samples"], s["frames"], s["g"]
    x = wd.shape_frames(s)
    with _plan(s, average=s["average"], segments_per_line=g) as plan:
        got = plan.rows(x)
        desc = assert_plan_ran(plan, L, F, welch=s["welch"])
        n = plan.row_length
    assert _form(desc) == tuple(s["form"]), desc
    got = np.asarray(got, np.float64).reshape(F, -1, n)
    rfs = wd.r_fullscale(N, L, wd.window_of(s))
    cols = wd.tone_columns(N, W, s["real"])
    failed = {}
    for f in range(F):
        ref = wlr.ref_lines(x[f], FS, N, 1, W, g, s["average"], wd.window_of(s))
        assert got[f].shape == ref.shape, (got[f].shape, ref.shape)
        r_got, r_ref = dr.row_amp(got[f]), dr.row_amp(ref)
        gate = wd.gate(FIX[s["name"]]["E32"][f])
        e = float(np.abs(r_got - r_ref).max() / rfs)
        tone = ", ".join(f"{j}: {np.abs(got[f][:, j] - ref[:, j]).max():+.4f} dB" for j in cols) or "outside the row"
        print(f"{wd.case_name(s, f)}: max |dr| {e:.3e} r_fs ({20 * np.log10(max(e, 1e-300)):.1f} dBc; "
              f"gate {gate:.3e}); weak tone bins {tone}")
        try:
            # check_rel divides by max |ref|; the gate is relative to a full-scale bin
            check_rel(r_got, r_ref, gate * rfs / r_ref.max(), f"welchdr/{s['form'][0]}/{s['form'][1]}/{s['kinds'][f]}",
                      wd.case_name(s, f))
        except AssertionError as exc:
            failed[wd.case_name(s, f)] = str(exc)
    assert sorted(failed) == _limited(s), (failed, _limited(s))
    if failed:
        raise GateMiss(failed)


# ----------------------------------------------------------------------------- non-finite values
# name: (shape, frames, frame that gets the NaN, frame that is zeroed); the name's first word is the FFT form
NONFINITE = {
    "stockham_256": (dict(n_fft=256, n_win=256, n_samples=768), 6, 1, 4),
    # four frames per workgroup: frame 1 shares its workgroup with 0, 2 and 3; frame 4 with 5
    "dif_1024": (dict(n_fft=1024, n_win=1024, n_samples=3072), 6, 1, 4),
    "dif_4096_split": (dict(n_fft=4096, n_win=4096, n_samples=5 * 4096), 1, 0, 0),
    "four_32768_fused_mean": (dict(n_fft=32768, n_win=32768, n_samples=3 * 32768), 6, 1, 4),
    "four_4096_means": (dict(n_fft=4096, n_win=4096, n_samples=4089, welch=2), 6, 1, 4),
}


@pytest.mark.parametrize("name", sorted(NONFINITE))
def test_zero_and_nan_frames(name):
    """An all-zero frame gives -inf in every column, a frame with one NaN sample NaN in every
    column (g = 1: in the lines of the segments that hold it, the other lines bytewise unchanged),
    and the other frames of the call keep their bytes, in all three detectors."""
    s, F, f_nan, f_zero = NONFINITE[name]
    N, W, L = s["n_fft"], s["n_win"], s["n_samples"]
    x = war.burst_frames(F, L, N, 1, W, 8800 + N)
    nper = min(N, L)
    step = nper - nper // 2
    nseg = (L - nper) // step + 1
    p = step + nper // 4 if nseg > 1 else L // 2          # inside segments 0 and 1, at their 3/4 and 1/4
    hit = [sg for sg in range(nseg) if sg * step <= p < sg * step + nper]
    xn, xz = x.copy(), x.copy()
    xn[f_nan, p] = np.nan
    xz[f_zero] = 0
    with _plan(s) as plan:
        for average in MODES:
            plan.set_average(average)
            for g in (0, 1):
                plan.set_segments_per_line(g)
                R = nseg if g else 1
                base = plan.rows(x).reshape(F, R, -1)
                desc = assert_plan_ran(plan, L, F, welch=s.get("welch", 0))
                assert desc.split()[0] == name.split("_")[0], desc
                if name == "dif_4096_split" and average == "mean" and g == 0:
                    assert desc.split()[1] == "parts", desc
                assert np.isfinite(base).all(), (name, average, g)
                zero = plan.rows(xz).reshape(F, R, -1)
                nan = plan.rows(xn).reshape(F, R, -1)
                assert np.all(np.isneginf(zero[f_zero])), (name, average, g, zero[f_zero])
                lines = hit if g else [0]
                assert np.isnan(nan[f_nan][lines]).all(), (name, average, g, np.isnan(nan[f_nan]).mean(axis=-1))
                for r in set(range(R)) - set(lines):
                    assert nan[f_nan][r].tobytes() == base[f_nan][r].tobytes(), (name, average, g, r)
                for f in range(F):
                    if f != f_zero:
                        assert zero[f].tobytes() == base[f].tobytes(), (name, average, g, "zero", f)
                    if f != f_nan:
                        assert nan[f].tobytes() == base[f].tobytes(), (name, average, g, "nan", f)


@pytest.mark.parametrize("F,first", [(16, "fc_decim"), (3, "pc_fir")], ids=["fc_runs_of_windows", "pc_tiles"])
def test_nan_frame_behind_the_decimators(F, first):
    """Zoom 8 in front of N = 1024: a NaN in frame 1 makes frame 1's mean row NaN and leaves every
    other frame's bytes alone.  Where the NaN spreads in frame 1's decimated IQ is not asserted
    (the reference's filtfilt poisons the whole frame, FC only the windows that hold it)."""
    from pypanadapter_amd import ZoomFFT
    N, zoom, W, L = 1024, 8, 128, 32773
    x = war.burst_frames(F, L, N, zoom, W, 8900)
    xn = x.copy()
    xn[1, L // 2 + 3] = np.nan
    with ZoomFFT(N, zoom, FS, n_win=W) as plan:
        plan.set_timing(True)
        base = plan.rows(x)
        names = plan.launch_names()
        assert first in names, names
        nan = plan.rows(xn)
    assert np.isfinite(base).all()
    assert np.isnan(nan[1]).all(), np.isnan(nan[1]).mean()
    for f in range(F):
        if f != 1:
            assert nan[f].tobytes() == base[f].tobytes(), f


# ----------------------------------------------------------------------------- scale invariance
@pytest.mark.parametrize("N,W,L,F", [(512, 512, 1536, 3), (4096, 4096, 8192, 3), (32768, 32768, 98304, 2)],
                         ids=["stockham512", "dif4096", "four32768"])
def test_rows_scale_exactly_with_the_input(N, W, L, F):
    """The sums, the scale and the one-sided factor scale exactly by a power of two (nothing
    under- or overflows at these magnitudes), so the row of 2^(+-12) x is the row of x shifted by
    +-40 * 12 log10(2) dB up to two roundings of log10f results and log10f's own last-place error:
    4 spacings of the largest |row|.  On unit noise, where every bin is far from zero."""
    x = war.burst_frames(F, L, N, 1, W, 9000 + N)
    with _plan(dict(n_fft=N, n_win=W)) as plan:
        row = plan.rows(x).astype(np.float64)
        assert_plan_ran(plan, L, F)
        for e in (12, -12):
            scaled = plan.rows(x * np.float32(2.0 ** e)).astype(np.float64)
            tol = 4 * np.spacing(np.float32(max(np.abs(row).max(), np.abs(scaled).max())))
            d = np.abs(scaled - (row + 40.0 * e * np.log10(2.0)))
            print(f"N = {N} x 2^{e}: max |row shift error| {d.max():.3e} dB (tolerance {tol:.3e})")
            assert d.max() <= tol, (N, e, float(d.max()), float(tol), int(d.argmax()))


# ----------------------------------------------------------------------------- the panadapter's own case
def _dc_frames(F, L, n_fft, zoom, n_win, in_dtype, seed):
    """A DC offset -- the RTL-SDR's spike, which f_lo = 1 Hz keeps inside the band at every zoom
    -- plus the p100 content: complex64 at amplitude 1, cu8 as the byte value 160 (0.255) with
    the content under one step of the converter and a dither of one step, so the bytes are 159,
    160 and 161.  Returns (what the plan receives, its value)."""
    from pypanadapter_amd import synth
    tone, noise = dr.LEVELS["p100"]
    x = np.stack([1.0 + synth.make_iq(L, FS, seed + f, n_fft=n_fft, zoom=zoom, n_win=n_win, f_lo=1.0,
                                      tones=[(0.31, tone)], noise=noise) for f in range(F)]).astype(np.complex64)
    if in_dtype == "complex64":
        return x, x
    dither = np.random.default_rng(seed).uniform(-1.0, 1.0, (F, 2 * L))
    b = np.clip(np.rint(160.0 + (x - 1.0).view(np.float32) * 127.5 + dither), 0, 255).astype(np.uint8)
    return b, (b.astype(np.float32) / np.float32(127.5) - np.float32(1.0)).view(np.complex64)


@pytest.mark.parametrize("in_dtype", ["complex64", "cu8"])
@pytest.mark.parametrize("zoom,N,F,path,kernel", [(2, 2048, 1, 4, "pc_tail"), (8, 1024, 16, 6, "fc_decim")],
                         ids=["zoom2_ui_default", "zoom8x16_fc"])
def test_dc_offset_end_to_end(oracle_lib, zoom, N, F, path, kernel, in_dtype):
    """The automatic schedule in front of Welch under a DC offset: per column
    |r_got - r_ref| <= (2 bound(path, case) + 8 E32) r_fs, bound from dynrange_ref.iq_bound with S
    and the FC truncation computed here on the CPU for this input, E32 on the oracle's decimated
    frame rounded to complex64."""
    from pypanadapter_amd import ZoomFFT
    W, L = N // zoom, dr.LENGTHS[zoom]
    raw, x = _dc_frames(F, L, N, zoom, W, in_dtype, 9300 + zoom)
    with ZoomFFT(N, zoom, FS, n_win=W, in_dtype=in_dtype) as plan:
        plan.set_timing(True)
        rows = plan.rows(raw)
        names = plan.launch_names()
        assert_plan_ran(plan, L, F)
    assert kernel in names and names[0] == kernel, names
    rows = rows.reshape(F, -1)
    for f in sorted({0, 1, F // 2, F - 1} & set(range(F))):
        c = dict(name=f"dc_{in_dtype}_z{zoom}_f{f}", zoom=zoom, fs=FS, f_lo=1.0, flip=False)
        rec = dict(S=dr.s_factor(c, x[f]), trunc=dr.trunc_terms(c, x[f]))
        bound = dr.iq_bound(path, c, rec)                     # asserts S <= S_CAP
        xd = oracle_lib.zoomfft(x[f], zoom, FS, 1.0).astype(np.complex64)
        E32 = wd.e32(xd, N, W)
        w = dr.welch_window(N, len(xd))
        A = float(np.abs(x[f]).max())
        rfs = dr.r_fullscale(A, FS, w)
        gate = 2.0 * bound + wd.gate(E32)
        ref = oracle_lib.psd_row(x[f], FS, N, zoom, W, "hamming", 1.0)
        r_got, r_ref = dr.row_amp(rows[f]), dr.row_amp(ref)
        e = float(np.abs(r_got - r_ref).max() / rfs)
        print(f"{c['name']}: max |dr| {e:.3e} r_fs ({20 * np.log10(max(e, 1e-300)):.1f} dBc; gate {gate:.3e} = "
              f"2 x {bound:.2e} (S {rec['S']:.2f}) + 8 x {E32:.2e})")
        check_rel(r_got, r_ref, gate * rfs / r_ref.max(), f"welchdr/e2e/zoom{zoom}/{in_dtype}", c["name"])
