// zfft_demod_plan.cpp -- the pure host side of the demodulator bank (zfft_demod_plan.h):
// choose_demod, demod_cut, the output counts, the design.  No HIP: built into libzfft.so and,
// stand-alone under ASan + UBSan, into tests/host/demod_form_sweep.cpp (which supplies set_error
// and links zfft_tap_plan.cpp for the design).
#include "zfft_demod_plan.h"

#include <algorithm>
#include <string>

namespace zfft {

void set_error(const std::string &msg);  // zfft_plan.cpp

namespace {

int lds_of(int kind, int lanes, int rows) { return 4 * lanes * (demod_row(rows - 1, kind) + 1); }

// The longest span, whole output steps, whose detected values and history fit `budget` bytes.
int span_of(int kind, int lanes, int halo, int Da, int budget) {
  int rows = budget / (4 * lanes);                          // the plain array's; a padded one holds fewer
  while (rows > 0 && lds_of(kind, lanes, rows) > budget) --rows;
  const int span = std::min(rows - halo, kDemodSpanMax);
  return span < Da ? 0 : span / Da * Da;
}

}  // namespace

bool demod_shape_ok(int K, int Ta, int Da) {
  return K >= 1 && K <= kDemodMaxStreams && Ta >= 1 && Ta <= kDemodMaxTaps && Da >= 1 && Da <= kDemodMaxDecim;
}

bool demod_strides_ok(int K, int64_t step_stride, int64_t stream_stride) {
  return step_stride >= 1 && step_stride <= kDemodMaxStride && stream_stride >= (K > 1 ? 1 : 0) &&
         stream_stride <= kDemodMaxStride;
}

DemodForm choose_demod(int K, int Ta, int Da, int64_t step_stride, int64_t stream_stride) {
  DemodForm f;
  if (!demod_shape_ok(K, Ta, Da) || !demod_strides_ok(K, step_stride, stream_stride)) return f;
  f.halo = Ta - 1;
  // neighbouring streams are neighbours in memory and a row of them is at least 64 bytes: lanes
  // along the streams; else one stream a tile, lanes along time
  f.kind = stream_stride == 1 && K >= kDemodLanesMin ? kDemodStreams : kDemodTime;
  int lanes = 1;
  if (f.kind == kDemodStreams) {
    while (lanes < K && lanes < kDemodLanesMax) lanes *= 2;
    // a span shorter than its history detects every sample more than twice: fewer streams, a
    // longer column
    while (lanes > kDemodLanesMin && span_of(f.kind, lanes, f.halo, Da, kDemodLdsWant) < std::max(f.halo, Da)) lanes /= 2;
  }
  int span = span_of(f.kind, lanes, f.halo, Da, kDemodLdsWant);
  if (span < std::max(f.halo, Da)) span = span_of(f.kind, lanes, f.halo, Da, kDemodLdsMax);
  if (span < Da) return f;  // (never: 8 lanes of 1023 + 64 rows are 34 KiB)
  f.lanes = lanes;
  f.span = span;
  f.outs = span / Da;
  f.lds_bytes = lds_of(f.kind, lanes, f.halo + span);
  f.stream_tiles = (K + lanes - 1) / lanes;
  return f;
}

DemodCut demod_cut(const DemodForm &f, uint64_t n0, int64_t steps, int Da) {
  DemodCut c;
  if (!f.ok() || steps < 1 || steps > kDemodMaxPush || n0 > kDemodMaxCount || Da < 1 || f.span != f.outs * Da) return c;
  c.nspans = (steps + f.span - 1) / f.span;
  c.ntiles = c.nspans * f.stream_tiles;
  c.outs = demod_steps(n0, steps, Da);
  c.r0 = (int)stream_first(n0, Da);
  c.grid = (int)std::min<int64_t>(c.ntiles, kDemodGridMax);
  return c;
}

}  // namespace zfft

using namespace zfft;

// Test hooks (not part of include/zfft.h; no plan, no device): the output count, and the form of a
// shape with the cut of a push -- form12 = {kind, lanes, outs, span, halo, lds_bytes, stream_tiles,
// nspans, ntiles, outputs, r0, grid}.
extern "C" int64_t zfft__demod_steps(uint64_t n0, int64_t steps, int32_t Da) { return demod_steps(n0, steps, Da); }
extern "C" int zfft__demod_form(int32_t K, int32_t Ta, int32_t Da, int64_t step_stride, int64_t stream_stride,
                                uint64_t n0, int64_t steps, int64_t *form12) {
  if (!form12) return -1;
  const DemodForm f = choose_demod(K, Ta, Da, step_stride, stream_stride);
  const DemodCut c = demod_cut(f, n0, steps, Da);
  if (!f.ok() || !c.ok()) return -1;
  const int64_t v[12] = {f.kind, f.lanes, f.outs, f.span, f.halo, f.lds_bytes, f.stream_tiles,
                         c.nspans, c.ntiles, c.outs, c.r0, c.grid};
  std::copy(v, v + 12, form12);
  return 0;
}

extern "C" int zfft_demod_design(int32_t n_taps, double cutoff, double beta, double *h_out) {
  if (n_taps < 1 || n_taps > kDemodMaxTaps) {
    set_error("demod_design: n_taps in [1, 1024]");
    return ZFFT_EINVAL;
  }
  return zfft_tap_design(n_taps, cutoff, beta, h_out);
}
