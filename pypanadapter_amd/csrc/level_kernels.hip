// level_kernels.hip -- the level bank's push (rule: zfft.h, zfft_plan_level; form and cut:
// zfft_level_plan.h).  Three launches a push, split where one workgroup needs
// what others produced:
//   peaks  every block of the key the push touches to its peak P (rule 3): the complete ones into
//          the push's peak rows behind the H + 2 carried ones, the running one into the next carry;
//   gains  the envelope E = max of H + 1 peaks by log-step doubling in LDS and the block gain G
//          (rule 4), once per block and lane;
//   apply  the step gain (rule 5) and the product (rule 6) on the delayed samples, the carried
//          ones first; then the next carry: the unemitted steps and the last H + 2 peaks.
// A push that emits nothing skips the gains.  All three work on the u axis of zfft_level_plan.h.
//
// Streams form (K >= 8): thread t is lane t mod lanes of row group t / lanes, so a wave's global
// loads and stores run along the lane axis; a row group walks `chunk` consecutive steps piece by
// piece, a piece lying in one block.  Time form (K < 8): the threads run along the (step, lane)
// elements, which are consecutive in memory at step_stride = K; the peaks reduce across a wave.
//
// What makes the outputs independent of the cut and of the form: a peak is a maximum of
// non-negative numbers that are never NaN, in any order the same; G is one division; a step's
// gain one subtraction and one fused multiply-add on exact operands; the output one product.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "zfft_level_plan.h"

namespace zfft {
namespace {

struct LevelGeom {
  int64_t u_in0, u_in1, e0u, e1u, nq, npk;
  int64_t x_stride, key_stride;  // in floats
  int64_t tiles, a_u0;
  int K, logB, H, ll, rows, chunk, piece, lane_tiles;
  int g_lanes, g_blocks, g_lane_tiles;
  float target, gmax, floor, squelch;
};

// One carry: (2 B - 1) K unemitted steps (row r being step e0u + r), K running peaks, (H + 2) K
// peaks of the blocks before the running one.
__device__ __forceinline__ int64_t carry_run(const LevelGeom &g) { return (int64_t)((2 << g.logB) - 1) * g.K; }
__device__ __forceinline__ int64_t carry_tail(const LevelGeom &g) { return carry_run(g) + g.K; }

// block q's peak of lane s is done: the running block's goes on to the next push
__device__ __forceinline__ void peak_store(const LevelGeom &g, int64_t q, int s, float m, const float *carry_old,
                                           float *carry_new, float *pk) {
  if (q == 2) m = fmaxf(m, carry_old[carry_run(g) + s]);  // the block the count lay in
  if (q < g.nq) pk[(q + g.H) * g.K + s] = m;
  else carry_new[carry_run(g) + s] = m;
}

// the carried peaks are the push's first H + 2 rows
__device__ __forceinline__ void peaks_head(const LevelGeom &g, const float *carry_old, float *pk) {
  const int64_t n = (int64_t)(g.H + 2) * g.K, step = (int64_t)gridDim.x * kLevelThreads;
  for (int64_t e = (int64_t)blockIdx.x * kLevelThreads + threadIdx.x; e < n; e += step) pk[e] = carry_old[carry_tail(g) + e];
}

__global__ void __launch_bounds__(kLevelThreads) level_peaks_streams_kernel(const float *__restrict__ key, LevelGeom g,
                                                                           const float *__restrict__ carry_old,
                                                                           float *__restrict__ carry_new,
                                                                           float *__restrict__ pk) {
  extern __shared__ __attribute__((aligned(16))) float ds[];
  const int tid = threadIdx.x, ll = g.ll, l = tid & ((1 << ll) - 1), rg = tid >> ll, nr = kLevelThreads >> ll;
  const int B = 1 << g.logB, per_rg = g.chunk / g.piece, per_block = B / g.piece, blocks = g.rows >> g.logB;
  for (int64_t tile = blockIdx.x; tile < g.tiles; tile += gridDim.x) {
    const int64_t rt = tile / g.lane_tiles;
    const int s = ((int)(tile - rt * g.lane_tiles) << ll) + l;
    const bool live = s < g.K;
    const int64_t ut0 = 2 * (int64_t)B + rt * g.rows;
    for (int pc = 0; pc < per_rg; ++pc) {
      const int64_t up = ut0 + rg * g.chunk + pc * g.piece;
      float m = 0.f;
      if (live && up < g.u_in1 && up + g.piece > g.u_in0) {
#pragma unroll 8
        for (int i = 0; i < g.piece; ++i) {
          const int64_t u = up + i;
          if (u >= g.u_in0 && u < g.u_in1) m = fmaxf(m, level_mag(key[(u - g.u_in0) * g.key_stride + s]));
        }
      }
      ds[((rg * per_rg + pc) << ll) + l] = m;
    }
    __syncthreads();
    for (int j = rg; j < blocks; j += nr) {
      const int64_t q = (ut0 >> g.logB) + j;
      if (live && q <= g.nq) {
        float m = 0.f;
        for (int k = 0; k < per_block; ++k) m = fmaxf(m, ds[((j * per_block + k) << ll) + l]);
        peak_store(g, q, s, m, carry_old, carry_new, pk);
      }
    }
    __syncthreads();  // the next tile overwrites the partial peaks
  }
  peaks_head(g, carry_old, pk);
}

__global__ void __launch_bounds__(kLevelThreads) level_peaks_time_kernel(const float *__restrict__ key, LevelGeom g,
                                                                        const float *__restrict__ carry_old,
                                                                        float *__restrict__ carry_new,
                                                                        float *__restrict__ pk) {
  constexpr int kMaxK = kLevelLanesMin - 1;
  const int tid = threadIdx.x, t = tid & 63, wave = tid >> 6;
  const int K = g.K, B = 1 << g.logB, seg = B < 64 ? B : 64;  // lanes of a wave that share a block
  for (int64_t tile = blockIdx.x; tile < g.tiles; tile += gridDim.x) {  // (one lane tile: a tile is a span)
    const int64_t ut0 = 2 * (int64_t)B + tile * g.rows;
    for (int64_t uc = ut0 + (int64_t)wave * g.chunk; uc < ut0 + g.rows; uc += (int64_t)(kLevelThreads / 64) * g.chunk) {
      float acc[kMaxK];
#pragma unroll
      for (int s = 0; s < kMaxK; ++s) acc[s] = 0.f;
      for (int64_t u = uc + t; u < uc + g.chunk; u += 64) {
        if (u >= g.u_in0 && u < g.u_in1) {
          const float *row = key + (u - g.u_in0) * g.key_stride;
#pragma unroll
          for (int s = 0; s < kMaxK; ++s)
            if (s < K) acc[s] = fmaxf(acc[s], level_mag(row[s]));
        }
      }
      for (int off = 1; off < seg; off <<= 1) {
#pragma unroll
        for (int s = 0; s < kMaxK; ++s) acc[s] = fmaxf(acc[s], __shfl_xor(acc[s], off));
      }
      const int64_t q = (uc + t) >> g.logB;
      if ((t & (seg - 1)) == 0 && q <= g.nq) {
#pragma unroll
        for (int s = 0; s < kMaxK; ++s)
          if (s < K) peak_store(g, q, s, acc[s], carry_old, carry_new, pk);
      }
    }
  }
  peaks_head(g, carry_old, pk);
}

// Both forms: a tile is g_blocks blocks of g_lanes lanes (any width: the divisions are one per
// peak, not per sample).  Row r of the tile is the push's peak row q0 + r, block q0 + r - H.
__global__ void __launch_bounds__(kLevelThreads) level_gains_kernel(const float *__restrict__ pk, LevelGeom g,
                                                                   float *__restrict__ gk) {
  extern __shared__ __attribute__((aligned(16))) float ds[];
  const int tid = threadIdx.x, W = g.g_lanes, H = g.H, K = g.K;
  const int n = (g.g_blocks + H) * W;
  for (int64_t tile = blockIdx.x; tile < g.tiles; tile += gridDim.x) {
    const int64_t bt = tile / g.g_lane_tiles, q0 = bt * g.g_blocks;
    const int s0 = (int)(tile - bt * g.g_lane_tiles) * W;
    float *src = ds, *dst = ds + n;
    for (int e = tid; e < n; e += kLevelThreads) {
      const int r = e / W, s = s0 + (e - r * W);
      src[e] = s < K && q0 + r < g.npk ? pk[(q0 + r) * K + s] : 0.f;
    }
    __syncthreads();
    // window maxima of 2, 4, ... rows ending at each row, from one copy into the other: a max
    // may take an operand twice, so overlapping windows need no care
    int k = 1;
    for (; 2 * k <= H + 1; k *= 2) {
      for (int e = tid; e < n; e += kLevelThreads) dst[e] = e >= k * W ? fmaxf(src[e], src[e - k * W]) : src[e];
      __syncthreads();
      float *t = src;
      src = dst, dst = t;
    }
    const int rest = H + 1 - k;  // the H + 1 rows are two windows of k, rest <= k apart
    for (int e = tid + H * W; e < n; e += kLevelThreads) {
      const int r = e / W, s = s0 + (e - r * W);
      const int64_t q = q0 + r - H;
      const float E = rest ? fmaxf(src[e], src[e - rest * W]) : src[e];
      if (s < K && q < g.nq) gk[q * K + s] = level_gain(E, g.target, g.gmax, g.floor, g.squelch);
    }
    __syncthreads();  // the next tile overwrites both copies
  }
}

// rule 5's ramp of block q for lane s: *g_lo and *d
__device__ __forceinline__ void level_ramp(const float *gk, int64_t q, int K, int s, float *g_lo, float *d) {
  const float g0 = gk[(q - 1) * K + s], g1 = gk[q * K + s], g2 = gk[(q + 1) * K + s];
  *g_lo = fminf(g0, g1);
  *d = __fsub_rn(fminf(g1, g2), *g_lo);
}

// step u of lane s: carried where it precedes the push
__device__ __forceinline__ float level_sample(const LevelGeom &g, const float *x, const float *carry_old, int64_t u, int s) {
  return u < g.u_in0 ? carry_old[(u - g.e0u) * g.K + s] : x[(u - g.u_in0) * g.x_stride + s];
}

// the next carry: the steps [e1u, u_in1) and the peaks of the last H + 2 complete blocks
__device__ __forceinline__ void level_carry(const LevelGeom &g, const float *x, const float *carry_old, float *carry_new,
                                            const float *pk) {
  const int64_t step = (int64_t)gridDim.x * kLevelThreads, first = (int64_t)blockIdx.x * kLevelThreads + threadIdx.x;
  const int64_t n = (g.u_in1 - g.e1u) * g.K;
  for (int64_t e = first; e < n; e += step) {
    const int64_t r = e / g.K;
    carry_new[e] = level_sample(g, x, carry_old, g.e1u + r, (int)(e - r * g.K));
  }
  const int64_t nt = (int64_t)(g.H + 2) * g.K, from = (g.npk - (g.H + 2)) * g.K;
  for (int64_t e = first; e < nt; e += step) carry_new[carry_tail(g) + e] = pk[from + e];
}

__global__ void __launch_bounds__(kLevelThreads) level_apply_streams_kernel(const float *__restrict__ x, LevelGeom g,
                                                                           const float *__restrict__ carry_old,
                                                                           float *__restrict__ carry_new,
                                                                           const float *__restrict__ pk,
                                                                           const float *__restrict__ gk,
                                                                           float *__restrict__ out) {
  const int tid = threadIdx.x, ll = g.ll, l = tid & ((1 << ll) - 1), rg = tid >> ll;
  const int B = 1 << g.logB, per_rg = g.chunk / g.piece;
  const float inv_b = 1.f / (float)B;  // exact
  for (int64_t tile = blockIdx.x; tile < g.tiles; tile += gridDim.x) {
    const int64_t rt = tile / g.lane_tiles;
    const int s = ((int)(tile - rt * g.lane_tiles) << ll) + l;
    if (s >= g.K) continue;
    const int64_t ut0 = g.a_u0 + rt * g.rows;
    for (int pc = 0; pc < per_rg; ++pc) {
      const int64_t up = ut0 + rg * g.chunk + pc * g.piece;
      if (up >= g.e1u || up + g.piece <= g.e0u) continue;
      const int i0 = (int)(up & (B - 1));
      float g_lo, d;
      level_ramp(gk, up >> g.logB, g.K, s, &g_lo, &d);
#pragma unroll 8
      for (int i = 0; i < g.piece; ++i) {
        const int64_t u = up + i;
        if (u >= g.e0u && u < g.e1u) {
          const float gain = __fmaf_rn((float)(i0 + i) * inv_b, d, g_lo);
          out[(u - g.e0u) * g.K + s] = __fmul_rn(gain, level_sample(g, x, carry_old, u, s));
        }
      }
    }
  }
  level_carry(g, x, carry_old, carry_new, pk);
}

__global__ void __launch_bounds__(kLevelThreads) level_apply_time_kernel(const float *__restrict__ x, LevelGeom g,
                                                                        const float *__restrict__ carry_old,
                                                                        float *__restrict__ carry_new,
                                                                        const float *__restrict__ pk,
                                                                        const float *__restrict__ gk,
                                                                        float *__restrict__ out) {
  const int tid = threadIdx.x, K = g.K, B = 1 << g.logB;
  const float inv_b = 1.f / (float)B;  // exact
  for (int64_t tile = blockIdx.x; tile < g.tiles; tile += gridDim.x) {  // (one lane tile: a tile is a span)
    const int64_t ut0 = g.a_u0 + tile * g.rows;
    const int64_t lo = ut0 > g.e0u ? ut0 : g.e0u, hi = ut0 + g.rows < g.e1u ? ut0 + g.rows : g.e1u;
    const int n = (int)(hi - lo) * K;
    for (int e = tid; e < n; e += kLevelThreads) {  // (output-major, lane-minor: the stores are consecutive)
      const int r = e / K, s = e - r * K;
      const int64_t u = lo + r;
      float g_lo, d;
      level_ramp(gk, u >> g.logB, K, s, &g_lo, &d);
      const float gain = __fmaf_rn((float)(int)(u & (B - 1)) * inv_b, d, g_lo);
      out[(lo - g.e0u) * K + e] = __fmul_rn(gain, level_sample(g, x, carry_old, u, s));
    }
  }
  level_carry(g, x, carry_old, carry_new, pk);
}

LevelGeom geom_of(const LevelForm &f, const LevelCut &c, int64_t x_stride, int64_t key_stride, const float par[4]) {
  int logb = 0, ll = 0;
  while ((1 << logb) < f.B) ++logb;
  while ((1 << ll) < f.lanes) ++ll;
  return LevelGeom{c.u_in0, c.u_in1, c.e0u, c.e1u, c.nq, c.npk, x_stride, key_stride, 0, c.a_u0, f.K, logb, f.H, ll, f.rows,
                   f.chunk, f.piece, f.lane_tiles, f.g_lanes, f.g_blocks, f.g_lane_tiles, par[0], par[1], par[2], par[3]};
}

// what the kernels' indexing relies on, whoever made the form and the cut
bool level_launch_ok(const LevelForm &f, const LevelCut &c) {
  if (!f.ok() || !c.ok() || !level_shape_ok(f.K, f.B, f.H)) return false;
  const bool streams = f.kind == kLevelStreams;
  const int64_t B = f.B, steps = c.u_in1 - c.u_in0;
  if (streams ? (f.lanes & (f.lanes - 1)) != 0 || f.lanes < kLevelLanesMin || f.lanes > kLevelLanesMax ||
                    f.chunk * (kLevelThreads / f.lanes) != f.rows || f.lds_bytes < 4 * f.lanes * (f.rows / f.piece)
              : f.lanes != f.K || f.K >= kLevelLanesMin || f.chunk != std::max(f.B, 64) ||
                    f.rows % (f.chunk * (kLevelThreads / 64)) != 0)
    return false;
  if (f.rows % f.B != 0 || f.piece != std::min(f.chunk, f.B) || f.chunk % f.piece != 0 ||
      f.lane_tiles != (f.K + f.lanes - 1) / f.lanes || f.lds_bytes > kLevelLdsMax)
    return false;
  if (f.g_lanes < 1 || f.g_blocks < 1 || f.g_lane_tiles != (f.K + f.g_lanes - 1) / f.g_lanes ||
      f.g_lds_bytes < 8 * f.g_lanes * (f.g_blocks + f.H) || f.g_lds_bytes > kLevelLdsMax)
    return false;
  if (steps < 1 || steps > kLevelMaxPush || c.u_in0 < 2 * B || c.u_in0 >= 3 * B || c.e0u < B || c.e0u > c.u_in0 ||
      c.u_in0 - c.e0u > 2 * B - 1 || c.e1u < c.e0u || c.e1u > c.u_in1 || c.u_in1 - c.e1u > 2 * B - 1 ||
      c.outs != c.e1u - c.e0u || c.nq != c.u_in1 / B || c.npk != c.nq + f.H || (c.outs > 0 && c.e1u != (c.nq - 1) * B))
    return false;
  const auto cdiv = [](int64_t a, int64_t d) { return (a + d - 1) / d; };
  return c.p_tiles == cdiv((c.nq - 1) * B, f.rows) * f.lane_tiles && c.p_grid >= 1 && c.p_grid <= c.p_tiles &&
         c.p_grid <= kLevelGridMax && c.g_grid <= kLevelGridMax && c.a_grid >= 1 && c.a_grid <= kLevelGridMax &&
         (c.outs > 0 ? c.g_tiles == cdiv(c.nq, f.g_blocks) * f.g_lane_tiles && c.g_grid >= 1 && c.a_u0 == c.e0u / B * B &&
                           c.a_tiles == cdiv(c.e1u - c.a_u0, f.rows) * f.lane_tiles
                     : c.g_tiles == 0 && c.a_tiles == 0);
}

}  // namespace

hipError_t launch_level_peaks(const float *key, int64_t key_stride, const LevelForm &f, const LevelCut &c,
                              const float *carry_old, float *carry_new, float *pk, hipStream_t st) {
  if (!level_launch_ok(f, c) || !level_stride_ok(f.K, key_stride)) return hipErrorInvalidValue;
  const float par[4] = {};
  LevelGeom g = geom_of(f, c, key_stride, key_stride, par);
  g.tiles = c.p_tiles;
  const dim3 grid((unsigned)c.p_grid), block(kLevelThreads);
  if (f.kind == kLevelStreams) level_peaks_streams_kernel<<<grid, block, f.lds_bytes, st>>>(key, g, carry_old, carry_new, pk);
  else level_peaks_time_kernel<<<grid, block, 0, st>>>(key, g, carry_old, carry_new, pk);
  return hipGetLastError();
}

hipError_t launch_level_gains(const LevelForm &f, const LevelCut &c, const float par[4], const float *pk, float *gk,
                              hipStream_t st) {
  if (!level_launch_ok(f, c) || c.g_tiles < 1 || !level_params_ok(par[0], par[1], par[2], par[3])) return hipErrorInvalidValue;
  LevelGeom g = geom_of(f, c, f.K, f.K, par);
  g.tiles = c.g_tiles;
  level_gains_kernel<<<dim3((unsigned)c.g_grid), dim3(kLevelThreads), f.g_lds_bytes, st>>>(pk, g, gk);
  return hipGetLastError();
}

hipError_t launch_level_apply(const float *x, int64_t x_stride, const LevelForm &f, const LevelCut &c, const float *carry_old,
                              float *carry_new, const float *pk, const float *gk, float *out, hipStream_t st) {
  if (!level_launch_ok(f, c) || !level_stride_ok(f.K, x_stride)) return hipErrorInvalidValue;
  const float par[4] = {};
  LevelGeom g = geom_of(f, c, x_stride, x_stride, par);
  g.tiles = c.a_tiles;
  const dim3 grid((unsigned)c.a_grid), block(kLevelThreads);
  if (f.kind == kLevelStreams) level_apply_streams_kernel<<<grid, block, 0, st>>>(x, g, carry_old, carry_new, pk, gk, out);
  else level_apply_time_kernel<<<grid, block, 0, st>>>(x, g, carry_old, carry_new, pk, gk, out);
  return hipGetLastError();
}

}  // namespace zfft
