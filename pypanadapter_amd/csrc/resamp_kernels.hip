// resamp_kernels.hip -- the resampler bank's push (rule: zfft.h, zfft_plan_resamp; form:
// zfft_resamp_plan.h).  One launch per push: a workgroup takes tiles round-robin,
// a tile being a span of input steps of `lanes` lanes.  It stages the span's samples and the
// T - 1 before them (from the carry where those precede the push) once each into LDS, writes its
// part of the next carry, and runs the polyphase FIR out of LDS.
//
// Streams form (K >= 8): thread t is lane l = t mod lanes of row group t / lanes, lane l being
// lane l of the tile, so a wave's global loads and stores run along the lane axis and its LDS
// reads along a row.  A row group works on one output at a time: with 64 lanes a row group is a
// wave, the output's phase is wave-uniform (the group's index goes through readfirstlane) and the
// T coefficients of that phase, one contiguous row of the phase-major table, are scalar loads that
// feed the multiply-adds as scalar operands.  Narrower tiles put 64 / lanes outputs in a wave and
// load the rows per lane.
//
// Time form (K < 8): a tile is a span of all K lanes and the 256 threads run along its outputs
// (output-major, lane-minor: the stores are consecutive).  Phases differ from thread to thread,
// so the whole table lives in LDS, phase-major with rows of an odd pitch.
//
// Order of operations (what makes the outputs independent of the cut and of the form): four
// partial sums, a_j over the k = j (mod 4) in ascending k from +0, one fused multiply-add of
// h[k L + phase] and x[i - k] each, then (a_0 + a_1) + (a_2 + a_3); exactly T products.  The S16
// format is one rounded product with the scale, then rint and the clamp.  Nothing in it depends on
// the tile, the lane, the form or the push.
#include <hip/hip_runtime.h>

#include "zfft_resamp_plan.h"

namespace zfft {
namespace {

struct ResampGeom {
  int64_t n;            // steps of the push
  int64_t ntiles;       // ResampCut's
  int64_t step_stride;  // in floats
  int K, L, M, T, p0;
  int lanes_log, span, halo, lane_tiles, pitch;
  float scale;
};

// rule 2: c(k) = h[k L + phase], d(k) = x[i - k]
template <class C, class D>
__device__ __forceinline__ float resamp_fir(int T, C c, D d) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int k = 0;
#pragma unroll 4
  for (; k + 4 <= T; k += 4) {
    a0 = __fmaf_rn(c(k), d(k), a0);
    a1 = __fmaf_rn(c(k + 1), d(k + 1), a1);
    a2 = __fmaf_rn(c(k + 2), d(k + 2), a2);
    a3 = __fmaf_rn(c(k + 3), d(k + 3), a3);
  }
  if (k < T) a0 = __fmaf_rn(c(k), d(k), a0);
  if (k + 1 < T) a1 = __fmaf_rn(c(k + 1), d(k + 1), a1);
  if (k + 2 < T) a2 = __fmaf_rn(c(k + 2), d(k + 2), a2);
  return __fadd_rn(__fadd_rn(a0, a1), __fadd_rn(a2, a3));
}

// rule 4
template <int FMT>
__device__ __forceinline__ void resamp_store(void *out, int64_t at, float y, float scale) {
  if (FMT == ZFFT_RESAMP_F32) {
    ((float *)out)[at] = y;
  } else {
    const float v = __fmul_rn(y, scale);
    // (the clamp first: rint of a bound is the bound, and the conversion sees a value it holds)
    ((short *)out)[at] = (short)(v != v ? 0 : __float2int_rn(fminf(fmaxf(v, -32768.f), 32767.f)));
  }
}

template <int FMT, bool WAVE>
__global__ void __launch_bounds__(kResampThreads) resamp_streams_kernel(const float *__restrict__ x, ResampGeom g,
                                                                       const float *__restrict__ hp,
                                                                       const float *__restrict__ carry_old,
                                                                       float *__restrict__ carry_new,
                                                                       void *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float ds[];
  // (a wave-wide tile knows its row pitch: the LDS reads take constant offsets)
  const int tid = threadIdx.x, ll = WAVE ? 6 : g.lanes_log, l = tid & ((1 << ll) - 1), nr = kResampThreads >> ll;
  const int rg = WAVE ? __builtin_amdgcn_readfirstlane(tid >> ll) : tid >> ll;
  const int K = g.K, L = g.L, M = g.M, T = g.T, H = g.halo;
  const int64_t keep0 = g.n - H;  // the next carry holds the steps from here on
  const int di = nr * M / L, dph = nr * M - di * L;  // a row group's next output: nr M further on the upsampled axis

  for (int64_t tile = blockIdx.x; tile < g.ntiles; tile += gridDim.x) {
    const int64_t b = tile / g.lane_tiles;
    const int s = ((int)(tile - b * g.lane_tiles) << ll) + l;
    const bool live = s < K;
    const int64_t s0 = b * g.span, s1 = s0 + g.span < g.n ? s0 + g.span : g.n;
    const int rows = H + (int)(s1 - s0);
    if (live) {
      // step p of the push (p >= -H): the carry's row H + p where it precedes the push
#pragma unroll 4
      for (int i = rg; i < rows; i += nr) {
        const int64_t p = s0 - H + i;
        const float v = p < 0 ? carry_old[(H + p) * K + s] : x[p * g.step_stride + s];
        ds[(i << ll) + l] = v;
        if (i >= H && p >= keep0) carry_new[(p - keep0) * K + s] = v;
      }
      // a push shorter than the carry: the rest of it is the old one's end
      if (b == 0)
        for (int64_t i = rg; i < -keep0; i += nr) carry_new[i * K + s] = carry_old[(i + g.n) * K + s];
    }
    __syncthreads();

    // the outputs j with s0 L <= p0 + j M < s1 L; output j0 + jj reads up to row rel / L of the span
    // at phase rel mod L, rel = p0 + (j0 + jj) M - s0 L < span L + M
    int64_t j0, j1;
    resamp_span_outs(s0, s1, g.p0, L, M, &j0, &j1);
    const int cnt = (int)(j1 - j0);
    const int rel = (int)(g.p0 + j0 * M - s0 * L) + rg * M;
    int i = rel / L, ph = rel - i * L;
    for (int jj = rg; jj < cnt; jj += nr) {  // (a lane past K runs along: the trip count stays the wave's)
      const float *c = hp + ph * T;
      const float *col = ds + ((i + H) << ll) + l;  // x[i]; i + H - k >= 0 for k < T
      const float y = resamp_fir(T, [&](int k) { return c[k]; }, [&](int k) { return col[-(k << ll)]; });
      if (live) resamp_store<FMT>(out, (j0 + jj) * K + s, y, g.scale);
      i += di, ph += dph;
      if (ph >= L) ph -= L, ++i;
    }
    __syncthreads();  // the next tile overwrites the columns
  }
}

template <int FMT>
__global__ void __launch_bounds__(kResampThreads) resamp_time_kernel(const float *__restrict__ x, ResampGeom g,
                                                                    const float *__restrict__ hp,
                                                                    const float *__restrict__ carry_old,
                                                                    float *__restrict__ carry_new,
                                                                    void *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float ds[];
  const int tid = threadIdx.x;
  const int K = g.K, L = g.L, M = g.M, T = g.T, H = g.halo, P = g.pitch;
  const int64_t keep0 = g.n - H;
  float *tab = ds, *xs = ds + L * P;
  // the table, once a workgroup (the first barrier of the loop below covers it); the pad is never read
  for (int e = tid; e < L * T; e += kResampThreads) {
    const int ph = e / T;
    tab[ph * P + (e - ph * T)] = hp[e];
  }

  for (int64_t tile = blockIdx.x; tile < g.ntiles; tile += gridDim.x) {  // (one lane tile: a tile is a span)
    const int64_t s0 = tile * g.span, s1 = s0 + g.span < g.n ? s0 + g.span : g.n;
    const int rows = H + (int)(s1 - s0);
    for (int e = tid; e < rows * K; e += kResampThreads) {
      const int i = e / K, s = e - i * K;
      const int64_t p = s0 - H + i;
      const float v = p < 0 ? carry_old[(H + p) * K + s] : x[p * g.step_stride + s];
      xs[e] = v;
      if (i >= H && p >= keep0) carry_new[(p - keep0) * K + s] = v;
    }
    if (tile == 0)
      for (int64_t e = tid; e < -keep0 * K; e += kResampThreads) carry_new[e] = carry_old[e + g.n * K];
    __syncthreads();

    int64_t j0, j1;
    resamp_span_outs(s0, s1, g.p0, L, M, &j0, &j1);
    const int cnt = (int)(j1 - j0), rel0 = (int)(g.p0 + j0 * M - s0 * L);
    for (int e = tid; e < cnt * K; e += kResampThreads) {
      const int jj = e / K, s = e - jj * K;
      const int rel = rel0 + jj * M, i = rel / L, ph = rel - i * L;
      const float *c = tab + ph * P;
      const float *col = xs + (i + H) * K + s;
      const float y = resamp_fir(T, [&](int k) { return c[k]; }, [&](int k) { return col[-k * K]; });
      resamp_store<FMT>(out, j0 * K + e, y, g.scale);
    }
    __syncthreads();  // the next tile overwrites the samples
  }
}

}  // namespace

hipError_t launch_resamp_push(const float *x, int64_t steps, int64_t step_stride, const ResampForm &f, const ResampCut &c,
                              int format, float scale, const float *hp, const float *carry_old, float *carry_new,
                              void *out, hipStream_t st) {
  int ll = 0;
  while ((1 << ll) < f.lanes) ++ll;
  const bool streams = f.kind == kResampStreams;
  if (!f.ok() || !c.ok() || !resamp_shape_ok(f.K, f.L, f.M, f.T) || !resamp_stride_ok(f.K, step_stride) || steps < 1 ||
      steps > kResampMaxPush || (format != ZFFT_RESAMP_F32 && format != ZFFT_RESAMP_S16) || f.halo != f.T - 1 ||
      f.span > kResampSpanMax || f.lds_bytes > kResampLdsMax ||
      (streams ? (1 << ll) != f.lanes || f.lanes < kResampLanesMin || f.lanes > kResampLanesMax || f.pitch != 0
               : f.lanes != f.K || f.K >= kResampLanesMin || f.pitch < f.T) ||
      f.lds_bytes < 4 * (f.L * f.pitch + f.lanes * (f.halo + f.span)) || f.lane_tiles != (f.K + f.lanes - 1) / f.lanes ||
      c.nspans != (steps + f.span - 1) / f.span || c.ntiles != c.nspans * f.lane_tiles || c.p0 < 0 || c.p0 >= f.M ||
      c.grid > c.ntiles || c.grid > kResampGridMax)
    return hipErrorInvalidValue;
  const ResampGeom g{steps, c.ntiles, step_stride, f.K, f.L, f.M, f.T, c.p0, ll, f.span, f.halo, f.lane_tiles, f.pitch, scale};
  const dim3 grid((unsigned)c.grid), block(kResampThreads);
  const bool s16 = format == ZFFT_RESAMP_S16;
#define ZFFT_RESAMP_LAUNCH(kernel) kernel<<<grid, block, f.lds_bytes, st>>>(x, g, hp, carry_old, carry_new, out)
  if (!streams) {
    if (s16) ZFFT_RESAMP_LAUNCH(resamp_time_kernel<ZFFT_RESAMP_S16>);
    else ZFFT_RESAMP_LAUNCH(resamp_time_kernel<ZFFT_RESAMP_F32>);
  } else if (f.lanes == kResampLanesMax) {
    if (s16) ZFFT_RESAMP_LAUNCH((resamp_streams_kernel<ZFFT_RESAMP_S16, true>));
    else ZFFT_RESAMP_LAUNCH((resamp_streams_kernel<ZFFT_RESAMP_F32, true>));
  } else {
    if (s16) ZFFT_RESAMP_LAUNCH((resamp_streams_kernel<ZFFT_RESAMP_S16, false>));
    else ZFFT_RESAMP_LAUNCH((resamp_streams_kernel<ZFFT_RESAMP_F32, false>));
  }
#undef ZFFT_RESAMP_LAUNCH
  return hipGetLastError();
}

}  // namespace zfft
