"""CPU checks of the Welch form chooser (csrc/zfft_welch_plan.cpp, no GPU needed).

* TABLE pins choose_welch through the zfft__welch_plan hook: every (n_fft, n_win, zoom, in_dtype,
  welch, average, segments_per_line, lines_route, cap_bytes, L, frames) -> the hook's rc and its
  description, or "refused" where zfft_plan_welch refuses the mode (ZFFT_EUNSUPPORTED above
  16384 points in one workgroup, ZFFT_EINVAL below 4096 in four steps).  The descriptions are
  written down from a transcription of the decisions the chooser replaced (process_device's
  G / R / four / fused / segs / split / chunk, the two split functions of the DIF kernel and
  welch_select's thresholds), not from the chooser; welch_plan_check.py ties the hook to the
  launches that actually run in the GPU tests.
* tests/host/welch_plan_sweep.cpp sweeps the chooser's domain for its invariants (every split
  part non-empty, chunks within the cap, the domain of each kernel form, byte counts) under
  ASan + UBSan, as a stand-alone program.

welch: 0 auto, 1 one workgroup per frame, 2 four-step.  average: 0 mean, 1 median, 2 max.
in_dtype: 0 complex64, 3 real f32 (one-sided rows at zoom 1)."""
import ctypes
import os
import shutil
import subprocess

ZFFT_EINVAL, ZFFT_EUNSUPPORTED = -1, -6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _d(fft, out, split, lines, chunk, select, last_split=None):
    return (f"{fft} {out} split={split} last_split={split if last_split is None else last_split} "
            f"lines={lines} chunk={chunk} select={select}")


def _row(fft, split, chunk):
    return _d(fft, "parts" if split > 1 else "row", split, 1, chunk, "none")


# (n_fft, n_win, zoom, in_dtype, welch, average, g, lines_route, cap_bytes, L, frames, rc, description)
TABLE = [
    # N on both sides of 1024, 4096 and 16384 (15 segments): one frame and a full batch
    (512, 64, 1, 0, 0, 0, 0, 0, 0, 4096, 1, 0, _row("stockham", 1, 1)),
    (512, 64, 1, 0, 0, 0, 0, 0, 0, 4096, 4096, 0, _row("stockham", 1, 4096)),
    (1024, 128, 1, 0, 0, 0, 0, 0, 0, 8192, 1, 0, _row("dif", 5, 1)),
    (1024, 128, 1, 0, 0, 0, 0, 0, 0, 8192, 4096, 0, _row("dif", 1, 4096)),
    (2048, 256, 1, 0, 0, 0, 0, 0, 0, 16384, 1, 0, _row("dif", 5, 1)),
    (2048, 256, 1, 0, 0, 0, 0, 0, 0, 16384, 4096, 0, _row("dif", 1, 4096)),
    (4096, 512, 1, 0, 0, 0, 0, 0, 0, 32768, 1, 0, _row("dif", 5, 1)),
    (4096, 512, 1, 0, 0, 0, 0, 0, 0, 32768, 4096, 0, _row("dif", 1, 4096)),
    (8192, 1024, 1, 0, 0, 0, 0, 0, 0, 65536, 1, 0, _row("dif", 5, 1)),
    (8192, 1024, 1, 0, 0, 0, 0, 0, 0, 65536, 4096, 0, _row("dif", 1, 4096)),
    (16384, 2048, 1, 0, 0, 0, 0, 0, 0, 131072, 1, 0, _row("dif", 5, 1)),
    (16384, 2048, 1, 0, 0, 0, 0, 0, 0, 131072, 4096, 0, _row("dif", 1, 4096)),
    (32768, 4096, 1, 0, 0, 0, 0, 0, 0, 262144, 1, 0, _row("four", 1, 1)),
    (32768, 4096, 1, 0, 0, 0, 0, 0, 0, 262144, 4096, 0, _row("four", 1, 4096)),
    # forced modes, and their refusals
    (4096, 512, 1, 0, 1, 0, 0, 0, 0, 32768, 2, 0, _row("dif", 5, 2)),
    (4096, 512, 1, 0, 2, 0, 0, 0, 0, 32768, 2, 0, _row("four", 1, 2)),
    (16384, 2048, 1, 0, 1, 0, 0, 0, 0, 131072, 2, 0, _row("dif", 5, 2)),
    (16384, 2048, 1, 0, 2, 0, 0, 0, 0, 131072, 2, 0, _row("four", 1, 2)),
    (32768, 4096, 1, 0, 2, 0, 0, 0, 0, 262144, 2, 0, _row("four", 1, 2)),
    (32768, 4096, 1, 0, 1, 0, 0, 0, 0, 262144, 2, ZFFT_EUNSUPPORTED, "refused"),
    (65536, 8192, 1, 0, 1, 0, 0, 0, 0, 524288, 2, ZFFT_EUNSUPPORTED, "refused"),
    (2048, 256, 1, 0, 2, 0, 0, 0, 0, 16384, 2, ZFFT_EINVAL, "refused"),
    (2048, 256, 1, 0, 1, 0, 0, 0, 0, 16384, 2, 0, _row("dif", 5, 2)),
    (512, 64, 1, 0, 2, 0, 0, 0, 0, 4096, 2, ZFFT_EINVAL, "refused"),
    (4096, 512, 1, 0, 2, 1, 0, 0, 0, 12288, 2, 0, _d("four", "segs", 1, 1, 2, "reg8")),
    (4096, 512, 1, 0, 1, 2, 0, 0, 0, 12288, 2, 0, _d("dif", "segs", 2, 1, 2, "reg8")),
    # short input (L_d = 624 < N): one segment of L_d samples, the Stockham kernel
    (2048, 2048, 512, 0, 0, 0, 0, 0, 0, 319488, 1, 0, _row("stockham", 1, 1)),
    (2048, 2048, 512, 0, 0, 0, 2, 0, 0, 319488, 1, 0, _row("stockham", 1, 1)),
    (2048, 2048, 512, 0, 0, 1, 0, 0, 0, 319488, 1, 0, _d("stockham", "segs", 1, 1, 1, "reg4")),
    (2048, 2048, 512, 0, 0, 1, 2, 0, 0, 319488, 1, 0, _d("stockham", "segs", 1, 1, 1, "reg4")),
    (2048, 2048, 512, 0, 0, 2, 0, 0, 0, 319488, 1, 0, _d("stockham", "segs", 1, 1, 1, "reg4")),
    (2048, 2048, 512, 0, 0, 2, 2, 0, 0, 319488, 1, 0, _d("stockham", "segs", 1, 1, 1, "reg4")),
    (8192, 1024, 512, 0, 0, 0, 0, 0, 0, 319488, 3, 0, _row("stockham", 1, 3)),
    (8192, 1024, 512, 0, 2, 1, 0, 0, 0, 319488, 3, 0, _d("four", "segs", 1, 1, 3, "reg4")),
    (1024, 1024, 1, 0, 1, 0, 0, 0, 0, 624, 1, 0, _row("stockham", 1, 1)),
    # nseg 1, 2, 3, 4, 5 at N = 1024, one frame: around the split floor (4 segments, 2 lines)
    (1024, 1024, 1, 0, 0, 0, 0, 0, 0, 1024, 1, 0, _row("dif", 1, 1)),
    (1024, 1024, 1, 0, 0, 1, 0, 0, 0, 1024, 1, 0, _d("dif", "segs", 1, 1, 1, "reg4")),
    (1024, 1024, 1, 0, 0, 0, 1, 0, 0, 1024, 1, 0, _row("dif", 1, 1)),
    (1024, 1024, 1, 0, 0, 0, 0, 0, 0, 1536, 1, 0, _row("dif", 1, 1)),
    (1024, 1024, 1, 0, 0, 1, 0, 0, 0, 1536, 1, 0, _d("dif", "segs", 1, 1, 1, "reg4")),
    (1024, 1024, 1, 0, 0, 0, 1, 0, 0, 1536, 1, 0, _d("dif", "lines", 2, 2, 1, "none")),
    (1024, 1024, 1, 0, 0, 0, 2, 0, 0, 1536, 1, 0, _row("dif", 1, 1)),
    (1024, 1024, 1, 0, 0, 0, 0, 0, 0, 2048, 1, 0, _row("dif", 1, 1)),
    (1024, 1024, 1, 0, 0, 1, 0, 0, 0, 2048, 1, 0, _d("dif", "segs", 1, 1, 1, "reg4")),
    (1024, 1024, 1, 0, 0, 0, 1, 0, 0, 2048, 1, 0, _d("dif", "lines", 3, 3, 1, "none")),
    (1024, 1024, 1, 0, 0, 0, 2, 0, 0, 2048, 1, 0, _d("dif", "lines", 2, 2, 1, "none")),
    (1024, 1024, 1, 0, 0, 0, 0, 0, 0, 2560, 1, 0, _row("dif", 2, 1)),
    (1024, 1024, 1, 0, 0, 1, 0, 0, 0, 2560, 1, 0, _d("dif", "segs", 2, 1, 1, "reg4")),
    (1024, 1024, 1, 0, 0, 0, 1, 0, 0, 2560, 1, 0, _d("dif", "lines", 4, 4, 1, "none")),
    (1024, 1024, 1, 0, 0, 0, 2, 0, 0, 2560, 1, 0, _d("dif", "lines", 2, 2, 1, "none")),
    (1024, 1024, 1, 0, 0, 0, 0, 0, 0, 3072, 1, 0, _row("dif", 2, 1)),
    (1024, 1024, 1, 0, 0, 1, 0, 0, 0, 3072, 1, 0, _d("dif", "segs", 2, 1, 1, "reg8")),
    (1024, 1024, 1, 0, 0, 0, 1, 0, 0, 3072, 1, 0, _d("dif", "lines", 5, 5, 1, "none")),
    (1024, 1024, 1, 0, 0, 0, 2, 0, 0, 3072, 1, 0, _d("dif", "lines", 3, 3, 1, "none")),
    # frames on both sides of the bound that fills the chip, each DIF size (8 segments):
    # mean, median and mean lines of 2 segments; then 2 frames
    (1024, 128, 1, 0, 0, 0, 0, 0, 0, 4608, 1532, 0, _row("dif", 3, 1532)),
    (1024, 128, 1, 0, 0, 1, 0, 0, 0, 4608, 1532, 0, _d("dif", "segs", 3, 1, 1532, "reg8")),
    (1024, 128, 1, 0, 0, 0, 2, 0, 0, 4608, 1532, 0, _d("dif", "lines", 2, 4, 1532, "none")),
    (1024, 128, 1, 0, 0, 0, 0, 0, 0, 4608, 1533, 0, _row("dif", 1, 1533)),
    (1024, 128, 1, 0, 0, 1, 0, 0, 0, 4608, 1533, 0, _d("dif", "segs", 1, 1, 1533, "reg8")),
    (1024, 128, 1, 0, 0, 0, 2, 0, 0, 4608, 1533, 0, _d("dif", "lines", 1, 4, 1533, "none")),
    (1024, 128, 1, 0, 0, 0, 0, 0, 0, 4608, 2, 0, _row("dif", 4, 2)),
    (1024, 128, 1, 0, 0, 0, 0, 0, 0, 4608, 511, 0, _row("dif", 4, 511)),
    (2048, 256, 1, 0, 0, 0, 0, 0, 0, 9216, 766, 0, _row("dif", 3, 766)),
    (2048, 256, 1, 0, 0, 1, 0, 0, 0, 9216, 766, 0, _d("dif", "segs", 3, 1, 766, "reg8")),
    (2048, 256, 1, 0, 0, 0, 2, 0, 0, 9216, 766, 0, _d("dif", "lines", 2, 4, 766, "none")),
    (2048, 256, 1, 0, 0, 0, 0, 0, 0, 9216, 767, 0, _row("dif", 1, 767)),
    (2048, 256, 1, 0, 0, 1, 0, 0, 0, 9216, 767, 0, _d("dif", "segs", 1, 1, 767, "reg8")),
    (2048, 256, 1, 0, 0, 0, 2, 0, 0, 9216, 767, 0, _d("dif", "lines", 1, 4, 767, "none")),
    (2048, 256, 1, 0, 0, 0, 0, 0, 0, 9216, 2, 0, _row("dif", 4, 2)),
    (4096, 512, 1, 0, 0, 0, 0, 0, 0, 18432, 383, 0, _row("dif", 3, 383)),
    (4096, 512, 1, 0, 0, 1, 0, 0, 0, 18432, 383, 0, _d("dif", "segs", 3, 1, 383, "reg8")),
    (4096, 512, 1, 0, 0, 0, 2, 0, 0, 18432, 383, 0, _d("dif", "lines", 2, 4, 383, "none")),
    (4096, 512, 1, 0, 0, 0, 0, 0, 0, 18432, 384, 0, _row("dif", 1, 384)),
    (4096, 512, 1, 0, 0, 1, 0, 0, 0, 18432, 384, 0, _d("dif", "segs", 1, 1, 384, "reg8")),
    (4096, 512, 1, 0, 0, 0, 2, 0, 0, 18432, 384, 0, _d("dif", "lines", 1, 4, 384, "none")),
    (4096, 512, 1, 0, 0, 0, 0, 0, 0, 18432, 2, 0, _row("dif", 4, 2)),
    (8192, 1024, 1, 0, 0, 0, 0, 0, 0, 36864, 191, 0, _row("dif", 3, 191)),
    (8192, 1024, 1, 0, 0, 1, 0, 0, 0, 36864, 191, 0, _d("dif", "segs", 3, 1, 191, "reg8")),
    (8192, 1024, 1, 0, 0, 0, 2, 0, 0, 36864, 191, 0, _d("dif", "lines", 2, 4, 191, "none")),
    (8192, 1024, 1, 0, 0, 0, 0, 0, 0, 36864, 192, 0, _row("dif", 1, 192)),
    (8192, 1024, 1, 0, 0, 1, 0, 0, 0, 36864, 192, 0, _d("dif", "segs", 1, 1, 192, "reg8")),
    (8192, 1024, 1, 0, 0, 0, 2, 0, 0, 36864, 192, 0, _d("dif", "lines", 1, 4, 192, "none")),
    (8192, 1024, 1, 0, 0, 0, 0, 0, 0, 36864, 2, 0, _row("dif", 4, 2)),
    (16384, 2048, 1, 0, 0, 0, 0, 0, 0, 73728, 95, 0, _row("dif", 3, 95)),
    (16384, 2048, 1, 0, 0, 1, 0, 0, 0, 73728, 95, 0, _d("dif", "segs", 3, 1, 95, "reg8")),
    (16384, 2048, 1, 0, 0, 0, 2, 0, 0, 73728, 95, 0, _d("dif", "lines", 2, 4, 95, "none")),
    (16384, 2048, 1, 0, 0, 0, 0, 0, 0, 73728, 96, 0, _row("dif", 1, 96)),
    (16384, 2048, 1, 0, 0, 1, 0, 0, 0, 73728, 96, 0, _d("dif", "segs", 1, 1, 96, "reg8")),
    (16384, 2048, 1, 0, 0, 0, 2, 0, 0, 73728, 96, 0, _d("dif", "lines", 1, 4, 96, "none")),
    (16384, 2048, 1, 0, 0, 0, 0, 0, 0, 73728, 2, 0, _row("dif", 4, 2)),
    # every detector, g in {0, 1, nseg - 1, nseg, nseg + 1}: DIF (17 segments) ...
    (1024, 1024, 1, 0, 0, 0, 0, 0, 0, 9216, 5, 0, _row("dif", 6, 5)),
    (1024, 1024, 1, 0, 0, 0, 1, 0, 0, 9216, 5, 0, _d("dif", "lines", 17, 17, 5, "none")),
    (1024, 1024, 1, 0, 0, 0, 16, 0, 0, 9216, 5, 0, _d("dif", "lines", 2, 2, 5, "none")),
    (1024, 1024, 1, 0, 0, 0, 17, 0, 0, 9216, 5, 0, _row("dif", 6, 5)),
    (1024, 1024, 1, 0, 0, 0, 18, 0, 0, 9216, 5, 0, _row("dif", 6, 5)),
    (1024, 1024, 1, 0, 0, 1, 0, 0, 0, 9216, 5, 0, _d("dif", "segs", 6, 1, 5, "reg24")),
    (1024, 1024, 1, 0, 0, 1, 1, 0, 0, 9216, 5, 0, _d("dif", "segs", 6, 17, 5, "reg4")),
    (1024, 1024, 1, 0, 0, 1, 16, 0, 0, 9216, 5, 0, _d("dif", "segs", 6, 2, 5, "reg16")),
    (1024, 1024, 1, 0, 0, 1, 17, 0, 0, 9216, 5, 0, _d("dif", "segs", 6, 1, 5, "reg24")),
    (1024, 1024, 1, 0, 0, 1, 18, 0, 0, 9216, 5, 0, _d("dif", "segs", 6, 1, 5, "reg24")),
    (1024, 1024, 1, 0, 0, 2, 0, 0, 0, 9216, 5, 0, _d("dif", "segs", 6, 1, 5, "reg24")),
    (1024, 1024, 1, 0, 0, 2, 1, 0, 0, 9216, 5, 0, _d("dif", "segs", 6, 17, 5, "reg4")),
    (1024, 1024, 1, 0, 0, 2, 16, 0, 0, 9216, 5, 0, _d("dif", "segs", 6, 2, 5, "reg16")),
    (1024, 1024, 1, 0, 0, 2, 17, 0, 0, 9216, 5, 0, _d("dif", "segs", 6, 1, 5, "reg24")),
    (1024, 1024, 1, 0, 0, 2, 18, 0, 0, 9216, 5, 0, _d("dif", "segs", 6, 1, 5, "reg24")),
    # ... Stockham (11 segments) ...
    (64, 64, 1, 0, 0, 0, 0, 0, 0, 384, 2, 0, _row("stockham", 1, 2)),
    (64, 64, 1, 0, 0, 0, 1, 0, 0, 384, 2, 0, _d("stockham", "segs", 1, 11, 2, "mean_lines")),
    (64, 64, 1, 0, 0, 0, 10, 0, 0, 384, 2, 0, _d("stockham", "segs", 1, 2, 2, "mean_lines")),
    (64, 64, 1, 0, 0, 0, 11, 0, 0, 384, 2, 0, _row("stockham", 1, 2)),
    (64, 64, 1, 0, 0, 0, 12, 0, 0, 384, 2, 0, _row("stockham", 1, 2)),
    (64, 64, 1, 0, 0, 1, 0, 0, 0, 384, 2, 0, _d("stockham", "segs", 1, 1, 2, "reg16")),
    (64, 64, 1, 0, 0, 1, 1, 0, 0, 384, 2, 0, _d("stockham", "segs", 1, 11, 2, "reg4")),
    (64, 64, 1, 0, 0, 1, 10, 0, 0, 384, 2, 0, _d("stockham", "segs", 1, 2, 2, "reg16")),
    (64, 64, 1, 0, 0, 1, 11, 0, 0, 384, 2, 0, _d("stockham", "segs", 1, 1, 2, "reg16")),
    (64, 64, 1, 0, 0, 1, 12, 0, 0, 384, 2, 0, _d("stockham", "segs", 1, 1, 2, "reg16")),
    (64, 64, 1, 0, 0, 2, 0, 0, 0, 384, 2, 0, _d("stockham", "segs", 1, 1, 2, "reg16")),
    (64, 64, 1, 0, 0, 2, 1, 0, 0, 384, 2, 0, _d("stockham", "segs", 1, 11, 2, "reg4")),
    (64, 64, 1, 0, 0, 2, 10, 0, 0, 384, 2, 0, _d("stockham", "segs", 1, 2, 2, "reg16")),
    (64, 64, 1, 0, 0, 2, 11, 0, 0, 384, 2, 0, _d("stockham", "segs", 1, 1, 2, "reg16")),
    (64, 64, 1, 0, 0, 2, 12, 0, 0, 384, 2, 0, _d("stockham", "segs", 1, 1, 2, "reg16")),
    # ... and four-step (5 segments)
    (32768, 4096, 1, 0, 0, 0, 0, 0, 0, 98304, 2, 0, _row("four", 1, 2)),
    (32768, 4096, 1, 0, 0, 0, 1, 0, 0, 98304, 2, 0, _d("four", "segs", 1, 5, 2, "mean_lines")),
    (32768, 4096, 1, 0, 0, 0, 4, 0, 0, 98304, 2, 0, _d("four", "segs", 1, 2, 2, "mean_lines")),
    (32768, 4096, 1, 0, 0, 0, 5, 0, 0, 98304, 2, 0, _row("four", 1, 2)),
    (32768, 4096, 1, 0, 0, 0, 6, 0, 0, 98304, 2, 0, _row("four", 1, 2)),
    (32768, 4096, 1, 0, 0, 1, 0, 0, 0, 98304, 2, 0, _d("four", "segs", 1, 1, 2, "reg8")),
    (32768, 4096, 1, 0, 0, 1, 1, 0, 0, 98304, 2, 0, _d("four", "segs", 1, 5, 2, "reg4")),
    (32768, 4096, 1, 0, 0, 1, 4, 0, 0, 98304, 2, 0, _d("four", "segs", 1, 2, 2, "reg4")),
    (32768, 4096, 1, 0, 0, 1, 5, 0, 0, 98304, 2, 0, _d("four", "segs", 1, 1, 2, "reg8")),
    (32768, 4096, 1, 0, 0, 1, 6, 0, 0, 98304, 2, 0, _d("four", "segs", 1, 1, 2, "reg8")),
    (32768, 4096, 1, 0, 0, 2, 0, 0, 0, 98304, 2, 0, _d("four", "segs", 1, 1, 2, "reg8")),
    (32768, 4096, 1, 0, 0, 2, 1, 0, 0, 98304, 2, 0, _d("four", "segs", 1, 5, 2, "reg4")),
    (32768, 4096, 1, 0, 0, 2, 4, 0, 0, 98304, 2, 0, _d("four", "segs", 1, 2, 2, "reg4")),
    (32768, 4096, 1, 0, 0, 2, 5, 0, 0, 98304, 2, 0, _d("four", "segs", 1, 1, 2, "reg8")),
    (32768, 4096, 1, 0, 0, 2, 6, 0, 0, 98304, 2, 0, _d("four", "segs", 1, 1, 2, "reg8")),
    # mean lines (11 segments, g = 4) fused or through the scratch: lines_route 0 / 1
    (512, 64, 1, 0, 0, 0, 4, 0, 0, 3072, 2, 0, _d("stockham", "segs", 1, 3, 2, "mean_lines")),
    (512, 64, 1, 0, 0, 0, 4, 1, 0, 3072, 2, 0, _d("stockham", "segs", 1, 3, 2, "mean_lines")),
    (1024, 128, 1, 0, 0, 0, 4, 0, 0, 6144, 2, 0, _d("dif", "lines", 3, 3, 2, "none")),
    (1024, 128, 1, 0, 0, 0, 4, 1, 0, 6144, 2, 0, _d("dif", "segs", 4, 3, 2, "mean_lines")),
    (16384, 2048, 1, 0, 0, 0, 4, 0, 0, 98304, 2, 0, _d("dif", "lines", 3, 3, 2, "none")),
    (16384, 2048, 1, 0, 0, 0, 4, 1, 0, 98304, 2, 0, _d("dif", "segs", 4, 3, 2, "mean_lines")),
    (32768, 4096, 1, 0, 0, 0, 4, 0, 0, 196608, 2, 0, _d("four", "segs", 1, 3, 2, "mean_lines")),
    (32768, 4096, 1, 0, 0, 0, 4, 1, 0, 196608, 2, 0, _d("four", "segs", 1, 3, 2, "mean_lines")),
    (4096, 512, 1, 0, 2, 0, 4, 0, 0, 20480, 2, 0, _d("four", "segs", 1, 3, 2, "mean_lines")),
    (1024, 1024, 1, 0, 0, 1, 4, 1, 0, 9216, 2, 0, _d("dif", "segs", 6, 5, 2, "reg4")),
    # selection, median: group sizes (600 segments) and segment counts around 4 .. 32 and 256
    (64, 50, 1, 0, 0, 1, 4, 0, 0, 19232, 2, 0, _d("stockham", "segs", 1, 150, 2, "reg4")),
    (64, 50, 1, 0, 0, 1, 5, 0, 0, 19232, 2, 0, _d("stockham", "segs", 1, 120, 2, "reg8")),
    (64, 50, 1, 0, 0, 1, 8, 0, 0, 19232, 2, 0, _d("stockham", "segs", 1, 75, 2, "reg8")),
    (64, 50, 1, 0, 0, 1, 9, 0, 0, 19232, 2, 0, _d("stockham", "segs", 1, 67, 2, "reg16")),
    (64, 50, 1, 0, 0, 1, 16, 0, 0, 19232, 2, 0, _d("stockham", "segs", 1, 38, 2, "reg16")),
    (64, 50, 1, 0, 0, 1, 17, 0, 0, 19232, 2, 0, _d("stockham", "segs", 1, 36, 2, "reg24")),
    (64, 50, 1, 0, 0, 1, 24, 0, 0, 19232, 2, 0, _d("stockham", "segs", 1, 25, 2, "reg24")),
    (64, 50, 1, 0, 0, 1, 25, 0, 0, 19232, 2, 0, _d("stockham", "segs", 1, 24, 2, "reg32")),
    (64, 50, 1, 0, 0, 1, 32, 0, 0, 19232, 2, 0, _d("stockham", "segs", 1, 19, 2, "reg32")),
    (64, 50, 1, 0, 0, 1, 33, 0, 0, 19232, 2, 0, _d("stockham", "segs", 1, 19, 2, "lds")),
    (64, 50, 1, 0, 0, 1, 256, 0, 0, 19232, 2, 0, _d("stockham", "segs", 1, 3, 2, "lds")),
    (64, 50, 1, 0, 0, 1, 257, 0, 0, 19232, 2, 0, _d("stockham", "segs", 1, 3, 2, "scratch")),
    (64, 50, 1, 0, 0, 1, 0, 0, 0, 160, 2, 0, _d("stockham", "segs", 1, 1, 2, "reg4")),
    (64, 50, 1, 0, 0, 1, 0, 0, 0, 192, 2, 0, _d("stockham", "segs", 1, 1, 2, "reg8")),
    (64, 50, 1, 0, 0, 1, 0, 0, 0, 288, 2, 0, _d("stockham", "segs", 1, 1, 2, "reg8")),
    (64, 50, 1, 0, 0, 1, 0, 0, 0, 320, 2, 0, _d("stockham", "segs", 1, 1, 2, "reg16")),
    (64, 50, 1, 0, 0, 1, 0, 0, 0, 544, 2, 0, _d("stockham", "segs", 1, 1, 2, "reg16")),
    (64, 50, 1, 0, 0, 1, 0, 0, 0, 576, 2, 0, _d("stockham", "segs", 1, 1, 2, "reg24")),
    (64, 50, 1, 0, 0, 1, 0, 0, 0, 800, 2, 0, _d("stockham", "segs", 1, 1, 2, "reg24")),
    (64, 50, 1, 0, 0, 1, 0, 0, 0, 832, 2, 0, _d("stockham", "segs", 1, 1, 2, "reg32")),
    (64, 50, 1, 0, 0, 1, 0, 0, 0, 1056, 2, 0, _d("stockham", "segs", 1, 1, 2, "reg32")),
    (64, 50, 1, 0, 0, 1, 0, 0, 0, 1088, 2, 0, _d("stockham", "segs", 1, 1, 2, "lds")),
    (64, 50, 1, 0, 0, 1, 0, 0, 0, 8224, 2, 0, _d("stockham", "segs", 1, 1, 2, "lds")),
    (64, 50, 1, 0, 0, 1, 0, 0, 0, 8256, 2, 0, _d("stockham", "segs", 1, 1, 2, "scratch")),
    # selection, max: no LDS form; and mean lines take their own kernel whatever the group size
    (64, 50, 1, 0, 0, 2, 4, 0, 0, 19232, 2, 0, _d("stockham", "segs", 1, 150, 2, "reg4")),
    (64, 50, 1, 0, 0, 2, 5, 0, 0, 19232, 2, 0, _d("stockham", "segs", 1, 120, 2, "reg8")),
    (64, 50, 1, 0, 0, 2, 32, 0, 0, 19232, 2, 0, _d("stockham", "segs", 1, 19, 2, "reg32")),
    (64, 50, 1, 0, 0, 2, 33, 0, 0, 19232, 2, 0, _d("stockham", "segs", 1, 19, 2, "scratch")),
    (64, 50, 1, 0, 0, 2, 256, 0, 0, 19232, 2, 0, _d("stockham", "segs", 1, 3, 2, "scratch")),
    (64, 50, 1, 0, 0, 2, 257, 0, 0, 19232, 2, 0, _d("stockham", "segs", 1, 3, 2, "scratch")),
    (64, 50, 1, 0, 0, 2, 0, 0, 0, 800, 2, 0, _d("stockham", "segs", 1, 1, 2, "reg24")),
    (64, 50, 1, 0, 0, 2, 0, 0, 0, 832, 2, 0, _d("stockham", "segs", 1, 1, 2, "reg32")),
    (64, 50, 1, 0, 0, 2, 0, 0, 0, 1056, 2, 0, _d("stockham", "segs", 1, 1, 2, "reg32")),
    (64, 50, 1, 0, 0, 2, 0, 0, 0, 1088, 2, 0, _d("stockham", "segs", 1, 1, 2, "scratch")),
    (64, 50, 1, 0, 0, 2, 0, 0, 0, 8224, 2, 0, _d("stockham", "segs", 1, 1, 2, "scratch")),
    (64, 50, 1, 0, 0, 2, 0, 0, 0, 8256, 2, 0, _d("stockham", "segs", 1, 1, 2, "scratch")),
    (64, 50, 1, 0, 0, 0, 33, 0, 0, 19232, 2, 0, _d("stockham", "segs", 1, 19, 2, "mean_lines")),
    # the scratch cap (one frame: 16384 B): chunks of 1, of 2 and of the whole call
    (1024, 1024, 1, 0, 0, 1, 0, 0, 0, 2560, 12, 0, _d("dif", "segs", 2, 1, 12, "reg4")),
    (1024, 1024, 1, 0, 0, 1, 0, 0, 16383, 2560, 12, 0, _d("dif", "segs", 2, 1, 1, "reg4")),
    (1024, 1024, 1, 0, 0, 1, 0, 0, 40960, 2560, 12, 0, _d("dif", "segs", 2, 1, 2, "reg4")),
    (1024, 1024, 1, 0, 0, 1, 0, 0, 196608, 2560, 12, 0, _d("dif", "segs", 2, 1, 12, "reg4")),
    (1024, 1024, 1, 0, 0, 1, 0, 0, 0, 2560, 7, 0, _d("dif", "segs", 2, 1, 7, "reg4")),
    (1024, 1024, 1, 0, 0, 1, 0, 0, 16383, 2560, 7, 0, _d("dif", "segs", 2, 1, 1, "reg4")),
    (1024, 1024, 1, 0, 0, 1, 0, 0, 40960, 2560, 7, 0, _d("dif", "segs", 2, 1, 2, "reg4")),
    (1024, 1024, 1, 0, 0, 2, 2, 0, 40960, 2560, 12, 0, _d("dif", "segs", 2, 2, 2, "reg4")),
    (1024, 1024, 1, 0, 0, 0, 2, 1, 40960, 2560, 12, 0, _d("dif", "segs", 2, 2, 2, "mean_lines")),
    (1024, 1024, 1, 0, 0, 0, 2, 0, 40960, 2560, 12, 0, _d("dif", "lines", 2, 2, 12, "none")),
    (512, 300, 1, 0, 0, 1, 0, 0, 15000, 1536, 7, 0, _d("stockham", "segs", 1, 1, 2, "reg8")),
    (4096, 512, 1, 0, 2, 1, 0, 0, 25600, 12288, 3, 0, _d("four", "segs", 1, 1, 2, "reg8")),
    (1024, 128, 4, 0, 0, 1, 0, 0, 0, 262144, 4096, 0, _d("dif", "segs", 1, 1, 4096, "lds")),
    # a last chunk of one frame splits its 400 segments further than the chunks of two
    (16384, 64, 1, 0, 0, 1, 0, 0, 256000, 3284992, 3, 0, _d("dif", "segs", 80, 1, 2, "scratch", last_split=134)),
    (16384, 64, 1, 0, 0, 1, 0, 0, 256000, 3284992, 4, 0, _d("dif", "segs", 80, 1, 2, "scratch")),
    # one-sided rows (real input at zoom 1)
    (1024, 301, 1, 3, 0, 0, 0, 0, 0, 9216, 2, 0, _row("dif", 6, 2)),
    (1024, 301, 1, 3, 0, 1, 0, 0, 0, 9216, 2, 0, _d("dif", "segs", 6, 1, 2, "reg24")),
    (1024, 301, 1, 3, 0, 2, 0, 0, 0, 9216, 2, 0, _d("dif", "segs", 6, 1, 2, "reg24")),
    (1024, 1024, 1, 3, 0, 0, 5, 0, 0, 9216, 2, 0, _d("dif", "lines", 4, 4, 2, "none")),
    # behind a decimator
    (4096, 512, 8, 0, 0, 0, 0, 0, 0, 98304, 1, 0, _row("dif", 2, 1)),
    (1024, 128, 8, 0, 0, 1, 0, 0, 0, 32768, 16, 0, _d("dif", "segs", 3, 1, 16, "reg8")),
    (1024, 128, 8, 0, 0, 0, 3, 0, 0, 32768, 16, 0, _d("dif", "lines", 3, 3, 16, "none")),
    (4096, 2048, 2, 0, 0, 0, 0, 0, 0, 299008, 1, 0, _row("dif", 36, 1)),
]


def _hook():
    from pypanadapter_amd import _lib as L, build
    build.build()
    f = L.load().zfft__welch_plan
    f.argtypes = [ctypes.c_int32] * 8 + [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_char_p,
                                         ctypes.c_int32]
    f.restype = ctypes.c_int
    return f


def welch_plan(n_fft, n_win, zoom, in_dtype, welch, average, g, lines_route, cap_bytes, L, frames):
    """(rc, description) of zfft__welch_plan."""
    buf = ctypes.create_string_buffer(128)
    rc = _hook()(n_fft, n_win, zoom, in_dtype, welch, average, g, lines_route, cap_bytes, L, frames, buf, len(buf))
    return rc, buf.value.decode()


def test_welch_plan_table():
    assert len(TABLE) == len({t[:11] for t in TABLE})  # no key twice
    wrong = []
    for *key, rc_want, want in TABLE:
        rc, desc = welch_plan(*key)
        if (rc, desc) != (rc_want, want):
            wrong.append((tuple(key), (rc_want, want), (rc, desc)))
    assert not wrong, wrong


def test_welch_plan_hook_arguments():
    ok = (1024, 128, 1, 0, 0, 0, 0, 0, 0, 8192, 1)
    assert welch_plan(*ok)[0] == 0
    for i, bad in ((0, 1000), (0, 16), (0, 131072), (1, 1), (1, 1025), (2, 3), (2, 1024), (3, 4), (3, -1), (5, 3),
                   (5, -1), (6, -1), (7, 2), (8, -1), (9, 0), (9, (1 << 30) + 1), (10, 0)):
        key = list(ok)
        key[i] = bad
        assert welch_plan(*key)[0] == ZFFT_EINVAL, key
    assert welch_plan(*ok[:4], 3, *ok[5:]) == (ZFFT_EINVAL, "refused")  # no such Welch mode
    buf = ctypes.create_string_buffer(4)  # a short buffer truncates, terminated
    assert _hook()(*ok, buf, 4) == 0 and buf.value == b"dif"


def test_welch_plan_sweep_sanitized(tmp_path):
    """The chooser over its domain as a stand-alone g++ program (no HIP, no Python in the child)
    under AddressSanitizer + UBSan: the invariants in tests/host/welch_plan_sweep.cpp."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/host/welch_plan_sweep.cpp"
    csrc = os.path.join(ROOT, "pypanadapter_amd", "csrc")
    exe = str(tmp_path / "welch_plan_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", csrc, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "welch_plan_sweep.cpp"),
                    os.path.join(csrc, "zfft_welch_plan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "welch_plan_sweep: ok" in r.stdout, r.stdout
