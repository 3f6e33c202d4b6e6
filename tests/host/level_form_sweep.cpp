// level_form_sweep.cpp -- stand-alone sweep of the level bank's pure host side
// (csrc/zfft_level_plan.cpp) over its domain, built with ASan + UBSan by tests/test_level_host.py:
// every (K, B, H) gets a form whose tiles are whole blocks, whose row groups' pieces lie in one
// block each, whose LDS requests are the sums of their parts and fit a launch, and whose lane tiles
// cover the K lanes once; for pushes at several counts and starts emitted() is rule 7's on 128-bit
// integers, the cut's u axis puts every carried step, every step of the push and every emitted
// step where the kernels index them (inside the carry, the push, the output, the peak and gain
// rows), the tiles of the three kernels cover their ranges, the grids are in range, and the steps
// of a cut stream sum to the whole's; outside the domain the chooser refuses.  No HIP, no plan.
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <limits>

#include "zfft_level_plan.h"

using namespace zfft;
using i128 = __int128;

static long g_bad = 0;
static void check(bool ok, const char *what, long long a, long long b, long long c) {
  if (ok) return;
  if (++g_bad <= 20) std::printf("FAIL %s: %lld %lld %lld\n", what, a, b, c);
}

static i128 emitted_ref(i128 N, i128 n_r, i128 B) {
  const i128 e = B * (N / B - 1);
  return e > n_r ? e : n_r;
}

int main() {
  long keys = 0;
  const uint64_t starts[] = {0, 1, 5, 8, 1023, ((uint64_t)1 << 32) - 100, ((uint64_t)1 << 40) + 3, ((uint64_t)1 << 62) - 1000000};
  const int64_t pushes[] = {1, 2, 7, 8, 9, 63, 64, 65, 1023, 1024, 2047, 2048, 2049, 4097, 20011, 300007, INT32_MAX};
  for (int K : {1, 2, 3, 5, 7, 8, 9, 16, 17, 63, 64, 65, 100, 1000, 2048})
    for (int B : {8, 16, 32, 64, 128, 256, 512, 1024})
      for (int H : {0, 1, 2, 3, 5, 40, 73, 127, 128, 1000, 4095, 4096}) {
        const LevelForm f = choose_level(K, B, H);
        ++keys;
        check(f.ok() && level_shape_ok(K, B, H), "a form for every shape", K, B, H);
        if (!f.ok()) continue;
        const bool streams = K >= kLevelLanesMin;
        check(f.kind == (streams ? kLevelStreams : kLevelTime) && f.K == K && f.B == B && f.H == H, "kind and shape", K, B, H);
        check(streams ? f.lanes >= kLevelLanesMin && f.lanes <= kLevelLanesMax && (f.lanes & (f.lanes - 1)) == 0 && f.lanes < 2 * K &&
                            f.chunk * (kLevelThreads / f.lanes) == f.rows && f.lds_bytes == 4 * f.lanes * (f.rows / f.piece)
                      : f.lanes == K && f.chunk == (B > 64 ? B : 64) && f.rows % (f.chunk * (kLevelThreads / 64)) == 0 && f.lds_bytes == 0,
              "lanes, chunk and LDS of the form", K, f.lanes, f.chunk);
        check(f.rows >= B && f.rows % B == 0 && f.rows >= kLevelTileRows && f.piece == (f.chunk < B ? f.chunk : B) && f.piece >= 1 &&
                  f.chunk % f.piece == 0 && B % f.piece == 0 && f.rows % f.chunk == 0,
              "a tile is whole blocks, a piece lies in one", f.rows, f.chunk, f.piece);
        check(f.lane_tiles * f.lanes >= K && (f.lane_tiles - 1) * f.lanes < K, "lane tiles cover K once", K, f.lanes, f.lane_tiles);
        check(f.g_lanes >= 1 && f.g_lanes <= f.lanes && f.g_blocks >= 1 && f.g_blocks <= kLevelGainRowsMax &&
                  f.g_lds_bytes == 8 * f.g_lanes * (f.g_blocks + H) && f.g_lds_bytes <= kLevelLdsMax && f.lds_bytes <= kLevelLdsMax &&
                  f.g_lane_tiles * f.g_lanes >= K && (f.g_lane_tiles - 1) * f.g_lanes < K,
              "the gains tile", f.g_lanes, f.g_blocks, f.g_lds_bytes);
        check(f.g_blocks >= (H / 2 > 16 ? H / 2 : 16) || f.g_lanes == 1, "a gains tile is not all history", H, f.g_lanes, f.g_blocks);
        if (K != 1 && K != 7 && K != 64 && K != 100 && K != 2048) continue;  // (the cuts depend on K through the tiles alone)
        for (uint64_t n_r : starts)
          for (uint64_t lead : {(uint64_t)0, (uint64_t)1, (uint64_t)B - 1, (uint64_t)B, (uint64_t)2 * B + 3, (uint64_t)100000}) {
            const uint64_t n0 = n_r + lead;
            for (int64_t n : pushes) {
              if (n0 + (uint64_t)n > kLevelMaxCount) continue;
              const LevelCut c = level_cut(f, n0, n_r, n);
              check(c.ok(), "a cut for every push", K, (long long)n, B);
              if (!c.ok()) continue;
              const i128 e0 = emitted_ref(n0, n_r, B), e1 = emitted_ref((i128)n0 + n, n_r, B);
              const i128 base = ((i128)(n0 / B) - 2) * B;
              check(level_emitted(n0, n_r, B) == (int64_t)e0 && level_emitted(n0 + n, n_r, B) == (int64_t)e1 &&
                        c.outs == (int64_t)(e1 - e0) && c.outs == level_steps(n0, n_r, n, B) && c.outs >= 0,
                    "emitted is rule 7's", (long long)n, B, (long long)c.outs);
              check(c.u_in0 == (int64_t)((i128)n0 - base) && c.u_in0 >= 2 * B && c.u_in0 < 3 * B && c.u_in1 == c.u_in0 + n &&
                        c.e0u == (int64_t)(e0 - base) && c.e1u == (int64_t)(e1 - base),
                    "the u axis", (long long)c.u_in0, (long long)c.e0u, (long long)c.e1u);
              // the carried steps [e0u, u_in0) and the next carry [e1u, u_in1) fit 2 B - 1 rows, and the emitted steps the output
              check(c.e0u >= B && c.e0u <= c.u_in0 && c.u_in0 - c.e0u <= 2 * B - 1 && c.e1u >= c.e0u && c.e1u <= c.u_in1 &&
                        c.u_in1 - c.e1u <= 2 * B - 1,
                    "the carries", (long long)c.e0u, (long long)c.e1u, (long long)c.u_in1);
              check(c.nq == c.u_in1 / B && c.nq >= 2 && c.npk == c.nq + H, "blocks of the push", (long long)c.nq, (long long)c.npk, H);
              if (c.outs > 0) {
                // an emitted step's block q has its neighbours' gains: 1 <= q, q + 1 < nq; and its H + 1 peaks: rows q .. q + H < npk
                const int64_t q_first = c.e0u / B, q_last = (c.e1u - 1) / B;
                check(q_first >= 1 && q_last + 1 < c.nq && c.e1u == (c.nq - 1) * B && q_last + 1 + H < c.npk, "gains of the emitted blocks",
                      (long long)q_first, (long long)q_last, (long long)c.nq);
                check(c.a_u0 == c.e0u / B * B && c.a_tiles == (c.e1u - c.a_u0 + f.rows - 1) / f.rows * f.lane_tiles &&
                          c.g_tiles == (c.nq + f.g_blocks - 1) / f.g_blocks * f.g_lane_tiles,
                      "tiles of the gains and the apply kernel", (long long)c.a_tiles, (long long)c.g_tiles, 0);
              } else {
                check(c.a_tiles == 0 && c.g_tiles == 0 && c.g_grid == 0, "nothing emitted, no gains", (long long)c.a_tiles,
                      (long long)c.g_tiles, c.g_grid);
              }
              // the peaks kernel's tiles cover blocks 2 .. nq, whose steps hold the whole push
              check(c.p_tiles == ((c.nq - 1) * B + f.rows - 1) / f.rows * f.lane_tiles && 2 * B <= c.u_in0 && c.u_in1 < (c.nq + 1) * B,
                    "tiles of the peaks kernel", (long long)c.p_tiles, (long long)c.nq, 0);
              check(c.p_grid >= 1 && c.p_grid <= kLevelGridMax && c.p_grid <= c.p_tiles && c.g_grid <= kLevelGridMax &&
                        c.g_grid <= c.g_tiles && c.a_grid >= 1 && c.a_grid <= kLevelGridMax,
                    "grids", c.p_grid, c.g_grid, c.a_grid);
            }
            // the steps of a cut stream are the whole's
            if (n0 + 5000 <= kLevelMaxCount) {
              int64_t sum = 0;
              uint64_t at = n0;
              for (int64_t n : {1, B - 1, B, B + 1, 2 * B - 1, 2 * B, 3, 775}) sum += level_steps(at, n_r, n, B), at += (uint64_t)n;
              check(sum == level_steps(n0, n_r, (int64_t)(at - n0), B), "the steps of a cut stream", B, (long long)sum, 0);
            }
          }
        for (int64_t n : {(int64_t)0, (int64_t)-1, (int64_t)INT32_MAX + 1}) check(!level_cut(f, 0, 0, n).ok(), "refused steps", K, (long long)n, 0);
        check(!level_cut(f, 5, 6, 5).ok() && !level_cut(f, ((uint64_t)1 << 62) - 2, 0, 5).ok() && level_cut(f, ((uint64_t)1 << 62) - 5, 0, 5).ok(),
              "refused counts", K, 0, 0);
      }
  // outside the domain
  for (int K : {0, -1, 2049}) check(!choose_level(K, 8, 0).ok() && !level_shape_ok(K, 8, 0), "refused K", K, 0, 0);
  for (int B : {0, -8, 1, 4, 12, 24, 1000, 2048}) check(!choose_level(4, B, 0).ok() && !level_shape_ok(4, B, 0), "refused B", B, 0, 0);
  for (int H : {-1, 4097}) check(!choose_level(4, 8, H).ok() && !level_shape_ok(4, 8, H), "refused H", H, 0, 0);
  check(level_params_ok(0.5f, 1e4f, 1e-6f, 0.f) && level_params_ok(kLevelCap, kLevelMin, kLevelCap, kLevelMin) &&
            !level_params_ok(0.f, 1.f, 1.f, 0.f) && !level_params_ok(1.f, 2 * kLevelCap, 1.f, 0.f) && !level_params_ok(1.f, 1.f, kLevelMin / 2, 0.f) &&
            !level_params_ok(1.f, 1.f, 1.f, -1.f) && !level_params_ok(1.f, 1.f, 1.f, kLevelMin / 2) && !level_params_ok(std::numeric_limits<float>::quiet_NaN(), 1.f, 1.f, 0.f),
        "refused levels", 0, 0, 0);
  check(level_stride_ok(4, 4) && level_stride_ok(4, kLevelMaxStride) && !level_stride_ok(4, 3) && !level_stride_ok(4, kLevelMaxStride + 1) &&
            !level_stride_ok(4, 0) && !level_stride_ok(4, -4),
        "refused strides", 0, 0, 0);
  check(level_steps(0, 0, -1, 8) == 0 && level_steps(5, 6, 5, 8) == 0 && level_steps(((uint64_t)1 << 62) + 1, 0, 5, 8) == 0, "refused steps of a push", 0, 0, 0);
  // rule 3 and rule 4 on the host, the meter's lines
  check(level_mag(-3.f) == 3.f && level_mag(std::numeric_limits<float>::quiet_NaN()) == 0.f && level_mag(std::numeric_limits<float>::infinity()) == kLevelCap && level_mag(-2 * kLevelCap) == kLevelCap && level_gain(0.f, 0.5f, 1e4f, 1e-6f, 0.f) == 1e4f &&
            level_gain(0.f, 0.5f, 1e4f, 1e-6f, 1e-3f) == 0.f && level_gain(1.f, 0.5f, 1e4f, 1e-6f, 1e-3f) == 0.5f,
        "magnitude and gain", 0, 0, 0);
  if (g_bad) {
    std::printf("level_form_sweep: %ld failures over %ld keys\n", g_bad, keys);
    return 1;
  }
  std::printf("level_form_sweep: ok (%ld keys)\n", keys);
  return 0;
}
