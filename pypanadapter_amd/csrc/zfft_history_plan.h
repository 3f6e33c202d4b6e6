// zfft_history_plan.h -- the row history's quantiser (rule in zfft.h, zfft_plan_history) and which
// form of the re-reduction (history_kernels.hip) a view takes, as values: pure host functions of
// the format, the levels and the window.  No HIP, no plan: zfft_history.cpp launches what
// choose_history returns, the launcher guards its invariants and tests/test_history_host.py
// sweeps both without a device.
#pragma once

#include <cstdint>

namespace zfft {

constexpr int kHistF32 = 0, kHistU16 = 1, kHistU8 = 2;  // enum zfft_history_format
constexpr int kHistWaves = 4;                           // waves per workgroup
constexpr int kHistLaneBytes = 16;                      // one load per lane and row
constexpr int kHistStrideQuantum = 16;                  // stored elements per row: a multiple of this

inline bool hist_format_ok(int format) { return format >= kHistF32 && format <= kHistU8; }
inline int hist_elem_bytes(int format) { return format == kHistF32 ? 4 : format == kHistU16 ? 2 : 1; }
// columns a lane holds per row (16 B), columns a wave holds per row
inline int hist_lane_cols(int format) { return kHistLaneBytes / hist_elem_bytes(format); }
inline int hist_tile_cols(int format) { return 64 * hist_lane_cols(format); }
// Elements per stored row: n rounded up to 16, so every row starts on a 16-byte boundary in
// every format and an aligned 16-byte load that begins inside a row ends inside its stored bytes.
inline int64_t hist_stride(int n) {
  return ((int64_t)n + kHistStrideQuantum - 1) / kHistStrideQuantum * kHistStrideQuantum;
}

// The quantiser's float32 constants (zfft.h): K codes above code 1, lo, inv = K / range and step
// = range / K, each division in double and rounded once.  F32: K = 0, the levels unused.
struct HistQuant {
  int format = kHistF32;
  int K = 0;
  float lo = 0.f, inv = 0.f, step = 0.f;
};
// false: a format outside the enum, or (U16 / U8) levels that are not finite with db_min < db_max
bool hist_quant(int format, double db_min, double db_max, HistQuant *q);
uint16_t hist_code(const HistQuant &q, float v);  // U16 / U8 only
float hist_value(const HistQuant &q, uint16_t code);

enum HistKind { kHistNone = 0, kHistWhole = 1, kHistSliced = 2 };

// A view of `lines` lines of m rows each over the columns [col0, col0 + span) into `width`
// pixels.  A workgroup of four waves owns one column tile -- px consecutive pixels whose buckets,
// with the up to lane_cols - 1 columns before col0's 16-byte boundary, fit the tile_cols columns
// a wave loads per row (px = 1 when one bucket alone is wider: its columns then fold onto the
// lane's accumulators) -- and
//   kHistWhole   the whole lines [y k, (y + 1) k) one after another, a line's rows dealt to the
//                four waves; s = 1;
//   kHistSliced  too few (line, tile) pairs to fill the chip and long groups: each line's m rows
//                are cut into s > 1 slices of slice_rows, one workgroup per (line, slice) writing
//                a partial to the plan's scratch; a finishing launch combines them.  k = 1.
struct HistForm {
  int kind = kHistNone;
  int px = 0, tiles = 0;      // pixels per tile, column tiles: grid.y
  int lines = 0;
  int k = 0;                  // lines per workgroup (whole)
  int s = 0, slice_rows = 0;  // slices per line and their rows (sliced)
  int gy = 0;                 // workgroups per tile: grid.x
  bool ok() const { return kind != kHistNone; }
};

// !ok() outside 1 <= lines <= 8192, 1 <= m <= 65536, 1 <= width <= span <= 65536, lines * width
// <= 2^25 and a format of the enum.
HistForm choose_history(int lines, int m, int span, int width, int format);

}  // namespace zfft
