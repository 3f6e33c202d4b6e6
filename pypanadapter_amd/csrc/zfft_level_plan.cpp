// zfft_level_plan.cpp -- the pure host side of the level bank (zfft_level_plan.h): choose_level,
// level_cut, emitted() and the per-push block ranges.  No HIP: built into libzfft.so and,
// stand-alone under ASan + UBSan, into tests/host/level_form_sweep.cpp.
#include "zfft_level_plan.h"

#include <algorithm>

namespace zfft {

bool level_shape_ok(int K, int B, int H) {
  return K >= 1 && K <= kLevelMaxLanes && B >= kLevelMinBlock && B <= kLevelMaxBlock && (B & (B - 1)) == 0 && H >= 0 &&
         H <= kLevelMaxHold;
}

bool level_params_ok(float target, float gmax, float floor, float squelch) {
  const auto in = [](float v) { return v >= kLevelMin && v <= kLevelCap; };
  return in(target) && in(gmax) && in(floor) && (squelch == 0.f || in(squelch));
}

bool level_stride_ok(int K, int64_t stride) { return stride >= K && stride <= kLevelMaxStride; }

int64_t level_emitted(uint64_t N, uint64_t n_r, int B) {
  if (B < 1 || N > kLevelMaxCount || n_r > N) return 0;
  return std::max((int64_t)n_r, (int64_t)B * ((int64_t)(N / (uint64_t)B) - 1));
}

int64_t level_steps(uint64_t n0, uint64_t n_r, int64_t steps, int B) {
  if (steps < 0 || steps > kLevelMaxPush || B < 1 || n0 > kLevelMaxCount || n_r > n0 || n0 + (uint64_t)steps > kLevelMaxCount)
    return 0;
  return level_emitted(n0 + (uint64_t)steps, n_r, B) - level_emitted(n0, n_r, B);
}

LevelForm choose_level(int K, int B, int H) {
  LevelForm f;
  if (!level_shape_ok(K, B, H)) return f;
  // a row of the lanes is at least 32 bytes: threads along the lane axis; else all K lanes in
  // one tile and the threads along time
  f.kind = K >= kLevelLanesMin ? kLevelStreams : kLevelTime;
  f.K = K, f.B = B, f.H = H;
  f.rows = std::max(B, kLevelTileRows);
  if (f.kind == kLevelStreams) {
    f.lanes = kLevelLanesMin;
    while (f.lanes < K && f.lanes < kLevelLanesMax) f.lanes *= 2;
    f.chunk = f.rows / (kLevelThreads / f.lanes);
    f.piece = std::min(f.chunk, B);
    f.lds_bytes = 4 * f.lanes * (f.rows / f.piece);
  } else {
    f.lanes = K;
    f.chunk = std::max(B, 64);
    f.piece = std::min(f.chunk, B);
    f.rows = std::max(f.rows, f.chunk * (kLevelThreads / 64));  // a wave takes a chunk at a time
    f.lds_bytes = 0;
  }
  f.lane_tiles = (K + f.lanes - 1) / f.lanes;
  // the gains tile: g_blocks + H rows of g_lanes peaks, twice.  A tile shorter than half its
  // history reads every peak more than three times: fewer lanes, a longer column; one lane fits
  // the longest hold (2 (4096 + 4096) floats).
  for (int w = f.lanes;; w = (w + 1) / 2) {
    const int rows = kLevelLdsMax / (8 * w);
    const int blocks = std::min(rows - H, kLevelGainRowsMax);
    if (blocks >= std::max(16, H / 2) || w == 1) {
      f.g_lanes = w;
      f.g_blocks = blocks;
      break;
    }
  }
  if (f.g_blocks < 1) return LevelForm{};  // (never: one lane has 8192 rows)
  f.g_lds_bytes = 8 * f.g_lanes * (f.g_blocks + H);
  f.g_lane_tiles = (K + f.g_lanes - 1) / f.g_lanes;
  return f;
}

LevelCut level_cut(const LevelForm &f, uint64_t n0, uint64_t n_r, int64_t steps) {
  LevelCut c;
  if (!f.ok() || steps < 1 || steps > kLevelMaxPush || n0 > kLevelMaxCount || n_r > n0 ||
      n0 + (uint64_t)steps > kLevelMaxCount)
    return c;
  const int64_t B = f.B;
  const int64_t cb0 = (int64_t)(n0 / (uint64_t)B), cb1 = (int64_t)((n0 + (uint64_t)steps) / (uint64_t)B);
  const int64_t base = (cb0 - 2) * B;  // (may be negative: the u axis starts two blocks before the count's)
  const int64_t e0 = level_emitted(n0, n_r, f.B), e1 = level_emitted(n0 + (uint64_t)steps, n_r, f.B);
  c.outs = e1 - e0;
  c.u_in0 = (int64_t)n0 - base;
  c.u_in1 = c.u_in0 + steps;
  c.e0u = e0 - base;
  c.e1u = e1 - base;
  c.nq = cb1 - cb0 + 2;
  c.npk = c.nq + f.H;
  const auto cdiv = [](int64_t a, int64_t d) { return (a + d - 1) / d; };
  c.p_tiles = cdiv((c.nq - 1) * B, f.rows) * f.lane_tiles;
  c.p_grid = (int)std::min<int64_t>(c.p_tiles, kLevelGridMax);
  if (c.outs > 0) {
    c.g_tiles = cdiv(c.nq, f.g_blocks) * f.g_lane_tiles;
    c.a_u0 = c.e0u / B * B;
    c.a_tiles = cdiv(c.e1u - c.a_u0, f.rows) * f.lane_tiles;
  }
  c.g_grid = (int)std::min<int64_t>(c.g_tiles, kLevelGridMax);
  // the next carry is written by every workgroup of the apply kernel, element by element
  const int64_t carry = (c.u_in1 - c.e1u + f.H + 2) * f.K;
  c.a_grid = (int)std::min<int64_t>(std::max<int64_t>(std::max<int64_t>(c.a_tiles, cdiv(carry, 4 * kLevelThreads)), 1), kLevelGridMax);
  return c;
}

}  // namespace zfft

using namespace zfft;

// Test hooks (not part of include/zfft.h; no plan, no device): emitted(), the steps of a push, and
// the form of a shape with the cut of a push -- form24 = {kind, lanes, rows, chunk, piece,
// lds_bytes, lane_tiles, g_lanes, g_blocks, g_lds_bytes, g_lane_tiles, outs, u_in0, u_in1, e0u,
// e1u, nq, npk, p_tiles, g_tiles, a_tiles, p_grid, g_grid, a_grid}.
extern "C" int64_t zfft__level_emitted(uint64_t N, uint64_t n_r, int32_t B) { return level_emitted(N, n_r, B); }
extern "C" int64_t zfft__level_steps(uint64_t n0, uint64_t n_r, int64_t steps, int32_t B) { return level_steps(n0, n_r, steps, B); }
extern "C" int zfft__level_form(int32_t K, int32_t B, int32_t H, uint64_t n0, uint64_t n_r, int64_t steps, int64_t *form24) {
  if (!form24) return -1;
  const LevelForm f = choose_level(K, B, H);
  const LevelCut c = level_cut(f, n0, n_r, steps);
  if (!f.ok() || !c.ok()) return -1;
  const int64_t v[24] = {f.kind, f.lanes, f.rows, f.chunk, f.piece, f.lds_bytes, f.lane_tiles, f.g_lanes, f.g_blocks,
                         f.g_lds_bytes, f.g_lane_tiles, c.outs, c.u_in0, c.u_in1, c.e0u, c.e1u, c.nq, c.npk,
                         c.p_tiles, c.g_tiles, c.a_tiles, c.p_grid, c.g_grid, c.a_grid};
  std::copy(v, v + 24, form24);
  return 0;
}
