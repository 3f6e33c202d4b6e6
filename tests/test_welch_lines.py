"""CPU checks of the time-resolved waterfall (zfft_plan_segments_per_line; no GPU needed): the
float64 reference helper the GPU tests use (welch_lines_ref.py) pinned against
scipy.signal.spectrogram and welch_average_ref.ref_row, and the plan-free entry points
zfft_line_count / zfft_line_times against the Python arithmetic and spectrogram's t."""
import ctypes

import numpy as np
import pytest
import scipy.signal as ss

import welch_average_ref as war
import welch_lines_ref as wlr

FS = war.FS
MODES = ("mean", "median", "max")
CASES = [(1024, 8, 128, 65536), (512, 2, 256, 8192), (64, 1, 64, 1344), (2048, 512, 2048, 319488),
         (32, 1, 31, 112)]


@pytest.mark.parametrize("N,zoom,W,L", CASES)
def test_reference_g1_is_scipy_spectrogram(oracle_lib, N, zoom, W, L):
    """g = 1: every line is one column of scipy.signal.spectrogram (welch's segments, no
    average) through the reference's fftshift, crop and dB, within 1e-12 dB, for every detector
    (a group of one: mean = median = max, bias(1) = 1)."""
    x = war.burst_frame(L, N, zoom, W, 7100 + N)
    xd = war.decimated(x, FS, zoom)
    nper = min(N, len(xd))
    _, t, S = ss.spectrogram(xd, FS, window="hamming", nperseg=nper, noverlap=nper // 2, nfft=N,
                             detrend="constant", return_onesided=False, scaling="density", mode="psd")
    want = np.stack([20 * np.log10(np.fft.fftshift(S[:, s])[N // 2 - W // 2: N // 2 + W // 2])
                     for s in range(S.shape[1])])
    for average in MODES:
        got = wlr.ref_lines(x, FS, N, zoom, W, 1, average)
        assert got.shape == want.shape == (war.nseg_of(L, N, zoom), 2 * (W // 2))
        assert np.abs(got - want).max() <= 1e-12


@pytest.mark.parametrize("N,zoom,W,L", CASES)
def test_reference_whole_frame_is_ref_row(oracle_lib, N, zoom, W, L):
    """g = 0, g = nseg and g > nseg: one line, welch_average_ref.ref_row exactly."""
    x = war.burst_frame(L, N, zoom, W, 7200 + N)
    nseg = war.nseg_of(L, N, zoom)
    for average in MODES:
        row = war.ref_row(x, FS, N, zoom, W, average)
        for g in (0, nseg, nseg + 1):
            got = wlr.ref_lines(x, FS, N, zoom, W, g, average)
            assert got.shape == (1,) + row.shape
            np.testing.assert_array_equal(got[0], row)


def test_reference_groups_and_tail(oracle_lib):
    """11 segments at g = 4: groups of 4, 4, 3, the median's bias that of each group's size."""
    N, W, L = 64, 64, 64 + 32 * 10
    x = war.burst_frame(L, N, 1, W, 7300)
    S = war.segment_psd(war.decimated(x, FS, 1), FS, N)
    assert S.shape[1] == 11
    for average in MODES:
        got = wlr.ref_lines(x, FS, N, 1, W, 4, average)
        assert got.shape == (3, W)
        for r, (a, b) in enumerate(((0, 4), (4, 8), (8, 11))):
            np.testing.assert_array_equal(got[r], wlr.crop_db(war.reduce_segments(S[:, a:b], average), N, W))


def _py_line_count(L, zoom, N, g):
    Ld = L
    for _ in range(int(np.log2(zoom))):
        Ld = (Ld + 1) // 2
    if Ld < N:
        return 1, 1
    nseg = (Ld - N) // (N - N // 2) + 1
    return wlr.line_count(nseg, g), nseg


def test_line_count_matches_python(zfft_lib):
    """Every residue of L mod 2 zoom, below and above n_fft decimated samples (below: the
    short-input branch, one line), g around nseg."""
    n = 0
    for zoom in (1, 2, 8, 64):
        for N in (32, 1024):
            for base in (N * zoom // 2, N * zoom, 5 * N * zoom):
                for res in range(2 * zoom):
                    L = base + res
                    _, nseg = _py_line_count(L, zoom, N, 0)
                    for g in sorted({0, 1, 2, 3, max(nseg - 1, 0), nseg, nseg + 1}):
                        want, _ = _py_line_count(L, zoom, N, g)
                        assert zfft_lib.zfft_line_count(L, zoom, N, g) == want, (L, zoom, N, g)
                        n += 1
    assert n >= 3 * 2 * (2 + 4 + 16 + 128) * 4  # every (base, N, residue), four values of g at least
    assert _py_line_count(32 * 64 // 2, 64, 32, 1) == (1, 1)  # L_d < N
    assert zfft_lib.zfft_line_count(9216, 1, 1024, 5) == 4  # 17 segments: 5, 5, 5, 2


def test_line_count_bad_arguments(zfft_lib):
    for args in ((0, 1, 32, 0), (-5, 1, 32, 0), (100, 3, 32, 0), (100, 0, 32, 0), (100, 1, 32, -1),
                 (100, 1, 0, 1)):
        assert zfft_lib.zfft_line_count(*args) == -1, args


def _line_times(lib, L, zoom, N, fs, g, cap):
    t = np.full(max(cap, 1), np.nan)
    count = ctypes.c_int32(-7)
    rc = lib.zfft_line_times(L, zoom, N, fs, g, t.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(count))
    return rc, count.value, t


@pytest.mark.parametrize("N,zoom,L", [(1024, 8, 65536), (64, 1, 64 + 32 * 10), (32, 1, 112), (512, 2, 8195),
                                      (2048, 512, 319488), (32, 1, 31 + 32)])
def test_line_times_match_spectrogram(zfft_lib, N, zoom, L):
    """The mean over each group of spectrogram's segment times, at the input rate, 1e-12
    relative; the short-input branch (L_d < N, odd L_d too) gives the one segment's centre."""
    nseg = war.nseg_of(L, N, zoom)
    for g in sorted({0, 1, 2, 3, 4, max(nseg - 1, 1), nseg, nseg + 3}):
        want = wlr.ref_line_times(L, FS, N, zoom, g)
        R = zfft_lib.zfft_line_count(L, zoom, N, g)
        assert R == len(want)
        rc, count, t = _line_times(zfft_lib, L, zoom, N, FS, g, R)
        assert (rc, count) == (0, R)
        np.testing.assert_allclose(t[:R], want, rtol=1e-12, atol=0)
        assert np.all(np.diff(t[:R]) > 0)
        if R > 1:  # a buffer one short: refused, nothing written, the count still reported
            from pypanadapter_amd import _lib
            rc, count, t = _line_times(zfft_lib, L, zoom, N, FS, g, R - 1)
            assert (rc, count) == (_lib.ZFFT_EINVAL, R)
            assert np.isnan(t).all()
            assert b"max" in zfft_lib.zfft_last_error()


def test_line_times_bad_arguments(zfft_lib):
    from pypanadapter_amd import _lib
    t = np.zeros(8)
    tp = t.ctypes.data_as(ctypes.c_void_p)
    count = ctypes.c_int32()
    cp = ctypes.byref(count)
    assert zfft_lib.zfft_line_times(9216, 1, 1024, FS, 5, None, 8, cp) == _lib.ZFFT_EINVAL
    assert zfft_lib.zfft_line_times(9216, 1, 1024, FS, 5, tp, 8, None) == _lib.ZFFT_EINVAL
    for args in ((9216, 1, 1024, FS, -1), (-1, 1, 1024, FS, 1), (9216, 3, 1024, FS, 1), (9216, 1, 1024, 0.0, 1),
                 (9216, 1, 1024, -FS, 1), (9216, 1, 1024, float("nan"), 1), (9216, 1, 0, FS, 1)):
        assert zfft_lib.zfft_line_times(*args, tp, 8, cp) == _lib.ZFFT_EINVAL, args
    assert zfft_lib.zfft_line_times(9216, 1, 1024, FS, 5, tp, 8, cp) == 0 and count.value == 4


def test_null_arguments_of_the_plan_entry_points(zfft_lib):
    """No plan and no ring: ZFFT_EINVAL, nothing dereferenced."""
    from pypanadapter_amd import _lib
    assert zfft_lib.zfft_plan_segments_per_line(None, 1) == _lib.ZFFT_EINVAL
    row = np.zeros(4, np.float32)
    produced = ctypes.c_int32()
    assert zfft_lib.zfft_ring_process_lines(None, None, row.ctypes.data_as(ctypes.c_void_p), 1,
                                            ctypes.byref(produced)) == _lib.ZFFT_EINVAL


def test_python_facade_argument_checks():
    import inspect

    from pypanadapter_amd import ZoomFFT, panadapter
    assert inspect.signature(ZoomFFT.__init__).parameters["segments_per_line"].default == 0
    sig = inspect.signature(panadapter.psd_lines)
    assert list(sig.parameters)[:5] == ["chunk", "fs", "fft_size", "fft_ratio", "segments_per_line"]
    assert sig.parameters["average"].default == "mean"
