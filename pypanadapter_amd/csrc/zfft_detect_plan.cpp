// zfft_detect_plan.cpp -- choose_detect (zfft_detect_plan.h): pure host code, built into
// libzfft.so and, stand-alone under ASan + UBSan, into tests/host/detect_form_sweep.cpp.
#include "zfft_detect_plan.h"

#include <algorithm>

namespace zfft {

namespace {
// (waves, per) in ascending domain order; detect_kernels.hip instantiates exactly these
constexpr int kForms[][2] = {{1, 1}, {1, 2}, {1, 4}, {1, 8}, {4, 8}, {16, 8}, {16, 64}};
// waves of a large call: ZFFT_DETECT_GRID_WAVES / 256 resident waves on each of 256 CUs
#ifndef ZFFT_DETECT_GRID_WAVES
#define ZFFT_DETECT_GRID_WAVES 8192
#endif
constexpr int kGridWaves = ZFFT_DETECT_GRID_WAVES;
}  // namespace

DetectForm choose_detect(int row_len, int count) {
  DetectForm f;
  if (row_len < 1 || row_len > kDetectMaxCols || count < 1) return f;
  for (const auto &wp : kForms)
    if (row_len <= kDetectWord * wp[0] * wp[1]) {
      f.waves = wp[0];
      f.per = wp[1];
      break;
    }
  f.grid = std::min(count, kGridWaves / f.waves);
  return f;
}

}  // namespace zfft

// Test hook (not part of include/zfft.h): the form of a call on `count` rows of row_len columns.
extern "C" int zfft__detect_form(int32_t row_len, int32_t count, int32_t *waves, int32_t *per, int32_t *grid) {
  const zfft::DetectForm f = zfft::choose_detect(row_len, count);
  if (!f.ok() || !waves || !per || !grid) return -1;
  *waves = f.waves;
  *per = f.per;
  *grid = f.grid;
  return 0;
}
