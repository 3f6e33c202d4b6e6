// zfft_history_plan.cpp -- the row history's quantiser and choose_history (zfft_history_plan.h):
// pure host code, built into libzfft.so.
#include "zfft_history_plan.h"

#include <algorithm>
#include <cmath>
#include <cstddef>

#include "zfft.h"
#include "zfft_view_plan.h"  // the viewport's geometry limits, which a view shares

namespace zfft {

namespace {
constexpr int kWholeGrid = 2048;   // workgroups of a large view: 8 of 4 waves on each of 256 CUs
constexpr int kSliceBelow = 512;   // fewer (line, tile) pairs than this: slice the lines
constexpr int kSliceGrid = 1024;   // workgroups a sliced view aims for
constexpr int kSliceMinRows = 32;  // rows per slice at least
}  // namespace

bool hist_quant(int format, double db_min, double db_max, HistQuant *q) {
  if (!hist_format_ok(format) || !q) return false;
  *q = HistQuant();
  q->format = format;
  if (format == kHistF32) return true;
  if (!std::isfinite(db_min) || !std::isfinite(db_max) || !(db_min < db_max)) return false;
  const double range = db_max - db_min;
  if (!std::isfinite(range)) return false;
  q->K = format == kHistU8 ? 254 : 65534;
  q->lo = (float)db_min;
  q->inv = (float)((double)q->K / range);
  q->step = (float)(range / (double)q->K);
  return true;
}

uint16_t hist_code(const HistQuant &q, float v) {
  if (v != v) return 0;
  const float d = v - q.lo;  // two roundings: a difference, then a product
  const float t = d * q.inv;
  return (uint16_t)(1 + (int)rintf(fminf(fmaxf(t, 0.f), (float)q.K)));
}

float hist_value(const HistQuant &q, uint16_t code) {
  if (code == 0) return std::nanf("");
  volatile float prod = (float)((int)code - 1) * q.step;  // rounded before the sum: never an fma
  return q.lo + prod;
}

HistForm choose_history(int lines, int m, int span, int width, int format) {
  HistForm f;
  if (!hist_format_ok(format) || lines < 1 || lines > kViewMaxHeight || m < 1 || m > kViewMaxGroup || width < 1 ||
      width > span || span > 65536 || (int64_t)lines * width > kViewMaxPixels)
    return f;
  const int bmax = (span + width - 1) / width;
  const int room = hist_tile_cols(format) - (hist_lane_cols(format) - 1);  // after the unaligned head
  f.px = bmax <= room ? std::min(width, room / bmax) : 1;
  f.tiles = (width + f.px - 1) / f.px;
  f.lines = lines;
  if ((int64_t)lines * f.tiles < kSliceBelow && m >= 4 * kSliceMinRows) {
    const int want = (int)std::max<int64_t>(2, kSliceGrid / ((int64_t)lines * f.tiles));
    const int s0 = std::min(want, m / kSliceMinRows);
    f.slice_rows = (m + s0 - 1) / s0;
    f.s = (m + f.slice_rows - 1) / f.slice_rows;  // (no empty last slice)
    if (f.s >= 2) {
      f.kind = kHistSliced;
      f.k = 1;
      f.gy = lines * f.s;
      return f;
    }
  }
  f.kind = kHistWhole;
  f.s = 1;
  f.slice_rows = m;
  const int ymax = std::max(1, kWholeGrid / f.tiles);
  f.k = (lines + ymax - 1) / ymax;
  f.gy = (lines + f.k - 1) / f.k;
  return f;
}

}  // namespace zfft

extern "C" int zfft_history_codes(int32_t format, double db_min, double db_max, const float *v, int64_t n,
                                  uint16_t *codes_out) {
  zfft::HistQuant q;
  if (format == zfft::kHistF32 || !zfft::hist_quant(format, db_min, db_max, &q) || n < 0 || (n > 0 && (!v || !codes_out)))
    return ZFFT_EINVAL;
  for (int64_t i = 0; i < n; ++i) codes_out[i] = zfft::hist_code(q, v[i]);
  return ZFFT_OK;
}

extern "C" int zfft_history_values(int32_t format, double db_min, double db_max, const uint16_t *codes, int64_t n,
                                   float *v_out) {
  zfft::HistQuant q;
  if (format == zfft::kHistF32 || !zfft::hist_quant(format, db_min, db_max, &q) || n < 0 || (n > 0 && (!codes || !v_out)))
    return ZFFT_EINVAL;
  for (int64_t i = 0; i < n; ++i) {
    if (codes[i] > q.K + 1) return ZFFT_EINVAL;
    v_out[i] = zfft::hist_value(q, codes[i]);
  }
  return ZFFT_OK;
}

// Test hook (not part of include/zfft.h): the form of a view, out[0..7] = kind, px, tiles, lines,
// k, s, slice_rows, gy; -1 where the chooser refuses.
extern "C" int zfft__history_form(int32_t lines, int32_t m, int32_t span, int32_t width, int32_t format,
                                  int32_t *out) {
  const zfft::HistForm f = zfft::choose_history(lines, m, span, width, format);
  if (!f.ok() || !out) return -1;
  const int v[8] = {f.kind, f.px, f.tiles, f.lines, f.k, f.s, f.slice_rows, f.gy};
  for (int i = 0; i < 8; ++i) out[i] = v[i];
  return 0;
}
