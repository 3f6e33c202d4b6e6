"""CPU checks of the Welch detectors (zfft_plan_average; no GPU needed): the host-side median
bias against scipy's, the float64 reference helper the GPU tests use (welch_average_ref.py)
pinned against the oracle and scipy.signal.welch, and the Python facade's argument checks."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.signal as ss
from scipy.signal._spectral_py import _median_bias

import welch_average_ref as war
from conftest import ROOT

FS = war.FS


def test_median_bias_matches_scipy_sanitized(tmp_path):
    """zfft::median_bias (csrc/zfft_median_bias.h) as a stand-alone g++ program under ASan +
    UBSan: n = 1 .. 300 within 1e-15 relative of scipy.signal's _median_bias."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/host/median_bias_main.cpp"
    exe = str(tmp_path / "median_bias")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "pypanadapter_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "median_bias_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, "300"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {int(a): float(b) for a, b in (ln.split() for ln in r.stdout.splitlines())}
    assert sorted(got) == list(range(1, 301))
    worst = max(abs(got[n] - _median_bias(n)) / _median_bias(n) for n in got)
    print(f"median_bias worst relative difference {worst:.2e}")
    assert worst <= 1e-15
    assert got[1] == 1.0 and got[2] == 1.0  # no term below n = 3


CASES = [(1024, 8, 128, 65536), (512, 2, 256, 8192), (64, 1, 64, 1344), (2048, 512, 2048, 319488),
         (32, 1, 31, 48)]


@pytest.mark.parametrize("N,zoom,W,L", CASES)
def test_reference_mean_is_the_pinned_oracle(oracle_lib, N, zoom, W, L):
    """The helper with the mean detector is coracle.psd_row (the pinned float64 oracle) within
    1e-9 dB: the same decimated IQ, scipy's segments in place of the oracle's own Welch."""
    x = war.burst_frame(L, N, zoom, W, 4100 + N)
    ref = oracle_lib.psd_row(x, FS, N, zoom, W)
    got = war.ref_row(x, FS, N, zoom, W, "mean")
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= 1e-9


@pytest.mark.parametrize("N,zoom,W,L", CASES)
def test_reference_median_is_scipy_welch_median(oracle_lib, N, zoom, W, L):
    """The helper with the median detector is scipy.signal.welch(average='median') on the same
    decimated IQ within 1e-12 relative (before the crop and the logarithm)."""
    x = war.burst_frame(L, N, zoom, W, 4200 + N)
    xd = war.decimated(x, FS, zoom)
    nper = min(N, len(xd))
    _, P = ss.welch(xd, FS, window="hamming", nperseg=nper, nfft=N, average="median",
                    return_onesided=False)
    mine = war.reduce_segments(war.segment_psd(xd, FS, N), "median")
    assert np.abs(mine - P).max() <= 1e-12 * P.max()
    row = war.ref_row(x, FS, N, zoom, W, "median")
    want = 20 * np.log10(np.fft.fftshift(P)[N // 2 - W // 2: N // 2 + W // 2])
    np.testing.assert_allclose(row, want, rtol=0, atol=1e-9)


def test_reference_onesided_median_is_scipy_welch_median():
    """Real input at zoom 1: welch's one-sided branch (doubled bins per segment)."""
    N, W, L = 1024, 301, 9216
    x = war.burst_frame(L, N, 1, W, 4300, real=True)
    _, P = ss.welch(x.astype(np.float64), FS, window="hamming", nperseg=N, nfft=N, average="median")
    want = 20 * np.log10(np.fft.fftshift(P)[N // 2 - W // 2: N // 2 + W // 2])
    row = war.ref_row(x, FS, N, 1, W, "median")
    assert row.shape == want.shape
    np.testing.assert_allclose(row, want, rtol=0, atol=1e-9)


def test_burst_separates_the_detectors(oracle_lib):
    """The test input does what it is for: at the burst's bins the median row sits tens of dB
    below the mean row and the max row above it."""
    N, zoom, W, L = 1024, 1, 1024, 9216  # 17 segments
    x = war.burst_frame(L, N, zoom, W, 4400)
    mean, med, mx = (war.ref_row(x, FS, N, zoom, W, a) for a in ("mean", "median", "max"))
    k = int(np.argmax(mean - med))
    assert mean[k] - med[k] > 40.0 and mx[k] - mean[k] > 10.0


def test_unknown_average_is_a_value_error(zfft_lib):
    from pypanadapter_amd import ZoomFFT, _lib, panadapter
    assert _lib.AVERAGES == {"mean": 0, "median": 1, "max": 2}
    with pytest.raises(ValueError):
        ZoomFFT(1024, 1, FS, average="mode")  # refused before a device is needed
    with pytest.raises(ValueError):
        panadapter.psd_row(np.zeros(2048, np.complex64), FS, 1024, 1, average="mode")
    assert zfft_lib.zfft_plan_average(None, 1) == _lib.ZFFT_EINVAL
