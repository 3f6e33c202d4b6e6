// zfft_detect_plan.h -- which form of the row detector (detect_kernels.hip; rule in zfft.h) a
// call takes, as a value: a pure host function of the row length and the rows per call.  No
// HIP, no plan: zfft_detect.cpp launches what it returns, the launcher guards its invariants
// and tests/test_detect_host.py sweeps it without a device.
#pragma once

#include <cstdint>

namespace zfft {

constexpr int kDetectMaxCols = 65536;  // n_win's upper bound
constexpr int kDetectMaxPerRow = 32;   // K, records per row
constexpr int kDetectWord = 64;        // columns per on-flag word: one wave's ballot

// One workgroup of `waves` waves holds a row in registers, `per` keys per lane: word
// wd = i * waves + wave (i < per) is the columns [64 wd, 64 wd + 64), lane l its column
// 64 wd + l, so a load is one coalesced 256-B line per wave and a ballot is a word.  A row has
// a wave boundary every 64 columns and a per-lane chunk boundary every 64 * waves.
struct DetectForm {
  int waves = 0, per = 0;
  int grid = 0;  // workgroups: each takes the rows blockIdx.x, blockIdx.x + grid, ...
  int cols() const { return kDetectWord * waves * per; }  // the form's domain: row_len <= cols()
  bool ok() const { return waves > 0; }
};

// The narrowest form whose domain holds row_len: one wave per row up to 512 columns (the UI's
// and cfg2's rows: no LDS traffic and no barrier in the selection), 4 waves up to 2048, 16
// waves (one 1024-thread workgroup) up to 65536.  The grid is one workgroup per row up to one
// resident round of the chip.  !ok() outside 1 <= row_len <= 65536 or count < 1.
DetectForm choose_detect(int row_len, int count);

}  // namespace zfft
