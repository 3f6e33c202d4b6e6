"""Float64 reference of the Welch detectors (zfft_plan_average) and the test inputs, shared by
tests/test_welch_average.py (CPU: the helper pinned against the oracle and scipy.signal.welch)
and tests/test_gpu_welch_average.py.

ref_row: oracle.coracle.zoomfft (complex128 decimated IQ), scipy.signal.spectrogram(mode='psd')
for the per-segment densities exactly as welch forms them (constant detrend, periodic window,
50 % overlap, nperseg = min(N, L_d), fs the original rate), the detector over the segments,
then the reference's fftshift, crop and 20 log10 (pypanadapter_spectrum.py:2111-2119)."""
import numpy as np
import scipy.signal as ss
from scipy.signal._spectral_py import _median_bias

from oracle import coracle
from pypanadapter_amd import synth

FS = 2.4e6


def segment_psd(xd, fs, n_fft, window="hamming", onesided=False):
    """(bins, nseg) float64 densities of the decimated frame xd."""
    nperseg = min(n_fft, len(xd))
    _, _, S = ss.spectrogram(xd, fs, window=window, nperseg=nperseg, noverlap=nperseg // 2,
                             nfft=n_fft, detrend="constant", return_onesided=onesided,
                             scaling="density", mode="psd")
    return S


def reduce_segments(S, average):
    if average == "mean":
        return S.mean(axis=-1)
    if average == "median":
        return np.median(S, axis=-1) / _median_bias(S.shape[-1])
    if average == "max":
        return S.max(axis=-1)
    raise ValueError(average)


def decimated(x, fs, zoom, f_lo=1.0):
    """The frame welch receives: real float64 for real input at zoom 1 (one-sided rows), else
    the oracle's complex128 zoomfft output."""
    x = np.asarray(x)
    if zoom == 1 and not np.iscomplexobj(x):
        return x.astype(np.float64)
    return coracle.zoomfft(x, zoom, fs, f_lo, mix=zoom > 1)


def ref_row(x, fs, n_fft, zoom, n_win, average, window="hamming", f_lo=1.0):
    xd = decimated(x, fs, zoom, f_lo)
    S = segment_psd(xd, fs, n_fft, window, onesided=not np.iscomplexobj(xd))
    P = np.fft.fftshift(reduce_segments(S, average))
    with np.errstate(divide="ignore"):
        return 20.0 * np.log10(np.abs(P[n_fft // 2 - n_win // 2: n_fft // 2 + n_win // 2]))


def nseg_of(L, n_fft, zoom):
    Ld = coracle.stage_lengths(L, zoom)[-1]
    nper = min(n_fft, Ld)
    return (Ld - nper) // (nper - nper // 2) + 1


def burst_frame(L, n_fft, zoom, n_win, seed, real=False, fs=FS):
    """The golden recipe (noise + two in-band tones, synth.make_iq) plus a burst of amplitude
    30 at an in-band frequency over a quarter of one segment (of n_fft * zoom input samples):
    it reaches one or two of the 50 %-overlapped segments, so the mean, the median and the max
    rows differ by tens of dB at its bins."""
    x = synth.make_iq(L, fs, seed, n_fft=n_fft, zoom=zoom, n_win=n_win).astype(np.complex128)
    seg = min(n_fft * zoom, L)
    nseg = nseg_of(L, n_fft, zoom)
    start = min((nseg // 3) * (seg // 2) + seg // 4, L - seg // 4)
    n = np.arange(start, start + seg // 4)
    hw = synth.display_halfwidth_hz(fs, n_fft, zoom, n_win)
    x[n] += synth.tone(n, 1.0 + 0.2 * hw, fs, 30.0)
    return x.real.astype(np.float32) if real else x.astype(np.complex64)


def burst_frames(F, L, n_fft, zoom, n_win, seed0, real=False):
    return np.stack([burst_frame(L, n_fft, zoom, n_win, seed0 + f, real) for f in range(F)])
