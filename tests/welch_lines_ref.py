"""Float64 reference of the time-resolved waterfall (zfft_plan_segments_per_line), shared by
tests/test_welch_lines.py (CPU: the helper pinned against scipy.signal.spectrogram and
welch_average_ref.ref_row) and tests/test_gpu_welch_lines.py.

ref_lines: welch_average_ref's decimated frame and per-segment densities, the segments in
groups of g consecutive ones (the last group holds the rest), each group through
reduce_segments -- so the median's bias is scipy's for that group's own size -- then the
reference's fftshift, crop and 20 log10 per line."""
import numpy as np

import welch_average_ref as war
from welch_average_ref import FS, burst_frames, decimated, nseg_of, reduce_segments, segment_psd  # noqa: F401


def line_count(nseg, g):
    """Rows per frame: 1 for g = 0 and g >= nseg, else ceil(nseg / g)."""
    return 1 if g <= 0 or g >= nseg else -(-nseg // g)


def crop_db(P, n_fft, n_win):
    P = np.fft.fftshift(P)
    with np.errstate(divide="ignore"):
        return 20.0 * np.log10(np.abs(P[n_fft // 2 - n_win // 2: n_fft // 2 + n_win // 2]))


def ref_lines(x, fs, n_fft, zoom, n_win, g, average, window="hamming", f_lo=1.0):
    """(R, row length) float64: the lines of one frame, in time order."""
    xd = decimated(x, fs, zoom, f_lo)
    S = segment_psd(xd, fs, n_fft, window, onesided=not np.iscomplexobj(xd))
    nseg = S.shape[-1]
    G = nseg if line_count(nseg, g) == 1 else g
    return np.stack([crop_db(reduce_segments(S[:, s0:s0 + G], average), n_fft, n_win)
                     for s0 in range(0, nseg, G)])


def ref_line_times(L, fs, n_fft, zoom, g):
    """Centre time of each line: scipy.signal.spectrogram's t of the decimated frame (rate
    fs / zoom ... given as t at rate 1, scaled by zoom / fs), averaged per group."""
    import scipy.signal as ss
    Ld = war.coracle.stage_lengths(L, zoom)[-1]
    nper = min(n_fft, Ld)
    _, t, _ = ss.spectrogram(np.zeros(Ld), 1.0, window="hamming", nperseg=nper, noverlap=nper // 2,
                             nfft=n_fft)
    nseg = len(t)
    G = nseg if line_count(nseg, g) == 1 else g
    return np.array([t[s0:s0 + G].mean() for s0 in range(0, nseg, G)]) * zoom / fs
