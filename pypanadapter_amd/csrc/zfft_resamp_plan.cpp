// zfft_resamp_plan.cpp -- the pure host side of the resampler bank (zfft_resamp_plan.h):
// choose_resamp, resamp_cut, the output count, the design.  No HIP: built into libzfft.so and,
// stand-alone under ASan + UBSan, into tests/host/resamp_form_sweep.cpp (which supplies set_error
// and links zfft_tap_plan.cpp for the design's formula).
#include "zfft_resamp_plan.h"

#include <algorithm>
#include <cmath>
#include <numeric>
#include <string>

#include "zfft_tap_plan.h"

namespace zfft {

void set_error(const std::string &msg);  // zfft_plan.cpp

namespace {

using u128 = unsigned __int128;

u128 ceil_div128(u128 a, uint64_t d) { return a / d + (a % d != 0); }

bool ratio_ok(int L, int M) {
  return L >= 1 && L <= kResampMaxL && M >= 1 && M <= kResampMaxM && std::gcd(L, M) == 1;
}

// The longest span whose samples, history and table fit `budget` bytes; <= 0 where none does.
int span_of(int lanes, int halo, int table_floats, int budget) {
  const int rows = (budget - 4 * table_floats) / (4 * lanes);
  return std::min(rows - halo, kResampSpanMax);
}

}  // namespace

bool resamp_shape_ok(int K, int L, int M, int T) {
  return K >= 1 && K <= kResampMaxLanes && ratio_ok(L, M) && T >= 1 && T <= kResampMaxT && L * T <= kResampMaxTable;
}

bool resamp_stride_ok(int K, int64_t step_stride) { return step_stride >= K && step_stride <= kResampMaxStride; }

int64_t resamp_steps(uint64_t n0, int64_t steps, int L, int M) {
  if (steps < 0 || steps > kResampMaxPush || n0 > kResampMaxCount || !ratio_ok(L, M)) return 0;
  const u128 a = (u128)n0 * (uint64_t)L, b = ((u128)n0 + (uint64_t)steps) * (uint64_t)L;
  return (int64_t)(ceil_div128(b, (uint64_t)M) - ceil_div128(a, (uint64_t)M));
}

int resamp_p0(uint64_t n0, int L, int M) {
  if (!ratio_ok(L, M)) return 0;
  const int r = (int)((u128)n0 * (uint64_t)L % (uint64_t)M);
  return r ? M - r : 0;
}

ResampForm choose_resamp(int K, int L, int M, int T, int64_t step_stride, int format) {
  ResampForm f;
  if (!resamp_shape_ok(K, L, M, T) || !resamp_stride_ok(K, step_stride) ||
      (format != ZFFT_RESAMP_F32 && format != ZFFT_RESAMP_S16))
    return f;
  const int halo = T - 1;
  // a row of the lanes is at least 32 bytes: lanes along the lane axis, every lane of a wave on
  // the same output; else all K lanes in one tile and the threads along its outputs, with the
  // table in LDS because their phases differ
  f.kind = K >= kResampLanesMin ? kResampStreams : kResampTime;
  int lanes = K, table = 0;
  if (f.kind == kResampStreams) {
    lanes = kResampLanesMin;
    while (lanes < K && lanes < kResampLanesMax) lanes *= 2;
    // a span shorter than its history stages every sample more than twice: fewer lanes, a longer column
    while (lanes > kResampLanesMin && span_of(lanes, halo, 0, kResampLdsWant) < std::max(halo, 1)) lanes /= 2;
  } else {
    f.pitch = T | 1;  // odd: the phases of a half wave spread over the 32 banks
    table = L * f.pitch;
  }
  int span = span_of(lanes, halo, table, kResampLdsWant);
  if (span < std::max(halo, 1)) span = span_of(lanes, halo, table, kResampLdsMax);
  if (span < 1) return f;  // (never: the table is at most 34 KiB, 7 lanes of 127 + 1 rows 4 KiB)
  // L > M: a step gives several outputs, and the output loop, not the staging, sizes the tile
  span = (int)std::min<int64_t>(span, std::max<int64_t>(1, (int64_t)kResampTileOuts * M / L));
  f.K = K, f.L = L, f.M = M, f.T = T;
  f.lanes = lanes;
  f.span = span;
  f.halo = halo;
  f.outs = (int)(((int64_t)span * L + M - 1) / M);
  f.lds_bytes = 4 * (table + lanes * (halo + span));
  f.lane_tiles = (K + lanes - 1) / lanes;
  return f;
}

ResampCut resamp_cut(const ResampForm &f, uint64_t n0, int64_t steps) {
  ResampCut c;
  if (!f.ok() || steps < 1 || steps > kResampMaxPush || n0 > kResampMaxCount || !ratio_ok(f.L, f.M)) return c;
  c.nspans = (steps + f.span - 1) / f.span;
  c.ntiles = c.nspans * f.lane_tiles;
  c.outs = resamp_steps(n0, steps, f.L, f.M);
  c.p0 = resamp_p0(n0, f.L, f.M);
  c.grid = (int)std::min<int64_t>(c.ntiles, kResampGridMax);
  return c;
}

}  // namespace zfft

using namespace zfft;

// Test hooks (not part of include/zfft.h; no plan, no device): the output count, and the form of a
// shape with the cut of a push -- form13 = {kind, lanes, span, halo, outs, pitch, lds_bytes,
// lane_tiles, nspans, ntiles, outputs, p0, grid}.
extern "C" int64_t zfft__resamp_steps(uint64_t n0, int64_t steps, int32_t L, int32_t M) { return resamp_steps(n0, steps, L, M); }
extern "C" int zfft__resamp_form(int32_t K, int32_t L, int32_t M, int32_t T, int64_t step_stride, int32_t format,
                                 uint64_t n0, int64_t steps, int64_t *form13) {
  if (!form13) return -1;
  const ResampForm f = choose_resamp(K, L, M, T, step_stride, format);
  const ResampCut c = resamp_cut(f, n0, steps);
  if (!f.ok() || !c.ok()) return -1;
  const int64_t v[13] = {f.kind, f.lanes, f.span, f.halo, f.outs, f.pitch, f.lds_bytes, f.lane_tiles,
                         c.nspans, c.ntiles, c.outs, c.p0, c.grid};
  std::copy(v, v + 13, form13);
  return 0;
}

extern "C" int zfft_resamp_design(int32_t L, int32_t M, int32_t taps_per_phase, double beta, double *h_out) {
  if (!h_out || !resamp_shape_ok(1, L, M, taps_per_phase) || !(beta >= 0.0) || !std::isfinite(beta)) {
    set_error("resamp_design: L in [1, 512], M in [1, 4096], gcd(L, M) = 1, taps_per_phase in [1, 128], "
              "L taps_per_phase <= 8192, beta >= 0");
    return ZFFT_EINVAL;
  }
  const int n = L * taps_per_phase;
  const int rc = kaiser_sinc(n, 0.4 / std::max(L, M), beta, h_out);
  if (rc) return rc;
  for (int k = 0; k < n; ++k) h_out[k] *= L;  // every phase has unit gain
  return ZFFT_OK;
}
