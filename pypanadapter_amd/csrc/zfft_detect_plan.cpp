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

DetectLocalForm choose_detect_local(int row_len, int n_win, int count, int half_window, int guard,
                                    size_t scratch_bytes) {
  DetectLocalForm f;
  if (!scratch_bytes) scratch_bytes = kDetectLocalScratch;
  if (row_len < 1 || n_win < row_len || n_win > kDetectMaxCols || count < 1 || half_window < 1 ||
      half_window > kDetectLocalMaxHalf || guard < 0 || guard > kDetectLocalMaxGuard ||
      scratch_bytes < (size_t)n_win * sizeof(float))
    return f;
  f.tile = kDetectLocalTile;
  f.tiles = (row_len + f.tile - 1) / f.tile;
  f.halo = guard + half_window;
  f.words = half_window <= 32 ? 1 : half_window <= 64 ? 2 : 4;
  f.chunk_rows = (int)std::min<size_t>((size_t)count, scratch_bytes / ((size_t)n_win * sizeof(float)));
  f.grid = (int)std::min<int64_t>((int64_t)f.chunk_rows * f.tiles, kDetectLocalGridMax);
  return f;
}

}  // namespace zfft

// Test hook (not part of include/zfft.h): the local floor's form, as
// {tile, tiles, halo, grid, chunk_rows, lds_keys, words}.
extern "C" int zfft__detect_local_form(int32_t row_len, int32_t n_win, int32_t count, int32_t half_window,
                                       int32_t guard, int64_t scratch_bytes, int32_t *out7) {
  if (!out7 || scratch_bytes < 0) return -1;
  const zfft::DetectLocalForm f =
      zfft::choose_detect_local(row_len, n_win, count, half_window, guard, (size_t)scratch_bytes);
  if (!f.ok()) return -1;
  out7[0] = f.tile, out7[1] = f.tiles, out7[2] = f.halo, out7[3] = f.grid, out7[4] = f.chunk_rows;
  out7[5] = f.lds_keys(), out7[6] = f.words;
  return 0;
}

// Test hook (not part of include/zfft.h): the form of a call on `count` rows of row_len columns.
extern "C" int zfft__detect_form(int32_t row_len, int32_t count, int32_t *waves, int32_t *per, int32_t *grid) {
  const zfft::DetectForm f = zfft::choose_detect(row_len, count);
  if (!f.ok() || !waves || !per || !grid) return -1;
  *waves = f.waves;
  *per = f.per;
  *grid = f.grid;
  return 0;
}
