// demod_kernels.hip -- the demodulator bank's push (rule: zfft.h, zfft_plan_demod; form:
// zfft_demod_plan.h).  One launch per push: a workgroup takes tiles round-robin,
// a tile being a span of input steps of `lanes` streams.  It detects the span's samples and the
// Ta - 1 before them (from the carry where those precede the push) once each into LDS, writes its
// part of the next carry, and runs the decimating FIR out of LDS.
//
// Mapping: thread t is lane l = t mod lanes of row group t / lanes.  In the streams form
// (lanes = 8 .. 64) lane l is stream l of the tile, so a wave's global loads and stores run along
// the stream axis and its LDS reads along a row; in the time form (lanes = 1) the 256 threads are
// 256 consecutive steps of one stream.  Both are the same code: the form is the tile's shape and
// the padding of the LDS column (demod_row).
//
// Order of operations (what makes the outputs independent of the cut and of the form): d is the
// fixed expression of rule 2 on x[n], x[n - 1] and n; the FIR is four partial sums, a_j over the
// k = j (mod 4) in ascending k, one fused multiply-add each, then (a_0 + a_1) + (a_2 + a_3).
// Nothing in it depends on the tile, the lane or the push.
#include <hip/hip_runtime.h>

#include "zfft_device.h"
#include "zfft_demod_plan.h"

namespace zfft {
namespace {

struct DemodGeom {
  int64_t n;                          // steps of the push
  int64_t nspans, ntiles;             // DemodCut's
  int64_t step_stride, stream_stride; // in complex samples
  uint32_t n0;                        // the count at the push's first step, mod 2^32
  int K, Ta, Da, r0;
  int lanes_log, span, halo, stream_tiles;
};

// exp(+2 pi i ph / 2^32) as (cos, sin): the high 24 bits are an exact float argument of sincospi,
// the low 8 a small angle e <= 2 pi 2^-24 (cos e = 1 to 7e-14, sin e = e)
__device__ __forceinline__ v2f demod_rot(uint32_t ph) {
  float s, c;
  sincospif((float)(ph >> 8) * 0x1p-23f, &s, &c);
  const float e = (float)(ph & 255u) * (float)(6.283185307179586 / 4294967296.0);
  return v2f{__fmaf_rn(-e, s, c), __fmaf_rn(e, c, s)};
}

// rule 2: the detected value of x[n] = c, x[n - 1] = pv (FM only) at count n (SSB only, mod 2^32)
__device__ __forceinline__ float demod_detect(uint32_t mode, uint32_t word, v2f c, v2f pv, uint32_t n) {
  if (mode == ZFFT_DEMOD_FM) {
    // z = x[n] conj(x[n - 1]): Re = c.x pv.x + c.y pv.y, Im = c.y pv.x - c.x pv.y
    const float re = __fmaf_rn(c.x, pv.x, __fmul_rn(c.y, pv.y));
    const float im = __fmaf_rn(c.y, pv.x, -__fmul_rn(c.x, pv.y));
    return re == 0.f && im == 0.f ? 0.f : __fmul_rn(atan2f(im, re), 0.318309886183790672f);
  }
  if (mode == ZFFT_DEMOD_SSB) {
    const v2f r = demod_rot(word * n);
    return __fmaf_rn(c.x, r.x, -__fmul_rn(c.y, r.y));
  }
  const float pw = __fmaf_rn(c.x, c.x, __fmul_rn(c.y, c.y));
  if (mode != ZFFT_DEMOD_AM) return pw;
  // sqrtf is the correctly rounded root (denormals included); __fsqrt_rn is the hardware's
  // approximation, one unit in the last place off in about one value of twenty-five.  Its
  // fix-up is some fifteen instructions: the empty asm keeps the compiler from computing it for
  // every mode and selecting, so a wave with no AM stream branches round it
  float v = pw;
  asm volatile("" : "+v"(v));
  return sqrtf(v);
}

template <int KIND>
__global__ void __launch_bounds__(kDemodThreads) demod_push_kernel(const v2f *__restrict__ x, DemodGeom g,
                                                                  const float *__restrict__ taps,
                                                                  const uint2 *__restrict__ par,
                                                                  const v2f *__restrict__ carry_old,
                                                                  v2f *__restrict__ carry_new,
                                                                  float *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float ds[];
  const int tid = threadIdx.x, ll = g.lanes_log, l = tid & ((1 << ll) - 1), rg = tid >> ll, nr = kDemodThreads >> ll;
  const int K = g.K, Ta = g.Ta, Da = g.Da, H = g.halo;
  const int64_t keep0 = g.n - Ta;  // the next carry holds the steps from here on

  for (int64_t tile = blockIdx.x; tile < g.ntiles; tile += gridDim.x) {
    const int64_t b = tile / g.stream_tiles;
    const int s = ((int)(tile - b * g.stream_tiles) << ll) + l;
    const bool live = s < K;
    const int64_t s0 = b * g.span, s1 = s0 + g.span < g.n ? s0 + g.span : g.n;
    const int rows = H + (int)(s1 - s0);
    if (live) {
      const uint2 ps = par[s];
      const bool fm = ps.x == ZFFT_DEMOD_FM;
      const v2f *xs = x + (int64_t)s * g.stream_stride;
      const v2f *co = carry_old + s;
      // step p of the push (p >= -Ta): the carry's row Ta + p where it precedes the push
      auto sample = [&](int64_t p) { return p < 0 ? co[(Ta + p) * K] : xs[p * g.step_stride]; };
#pragma unroll 4
      for (int i = rg; i < rows; i += nr) {
        const int64_t p = s0 - H + i;
        const v2f c = sample(p);
        const v2f pv = fm ? sample(p - 1) : splat(0.f);
        ds[(demod_row(i, KIND) << ll) + l] = demod_detect(ps.x, ps.y, c, pv, g.n0 + (uint32_t)p);
        if (i >= H && p >= keep0) carry_new[(p - keep0) * K + s] = c;
      }
      // a push shorter than the carry: the rest of it is the old one's end
      if (b == 0)
        for (int64_t i = rg; i < -keep0; i += nr) carry_new[i * K + s] = co[(i + g.n) * K];
    }
    __syncthreads();

    // the outputs j with s0 <= r0 + j Da < s1
    int64_t j0, j1;
    demod_span_outs(s0, s1, g.r0, Da, &j0, &j1);
    const int cnt = live ? (int)(j1 - j0) : 0;
    for (int jj = rg; jj < cnt; jj += nr) {
      const int64_t j = j0 + jj;
      const int i0 = (int)(g.r0 + j * Da - s0) + H;  // d[m Da] in the column; i0 - k >= 0 for k < Ta
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      auto d = [&](int k) { return ds[(demod_row(i0 - k, KIND) << ll) + l]; };
      int k = 0;
      for (; k + 4 <= Ta; k += 4) {
        a0 = __fmaf_rn(taps[k], d(k), a0);
        a1 = __fmaf_rn(taps[k + 1], d(k + 1), a1);
        a2 = __fmaf_rn(taps[k + 2], d(k + 2), a2);
        a3 = __fmaf_rn(taps[k + 3], d(k + 3), a3);
      }
      if (k < Ta) a0 = __fmaf_rn(taps[k], d(k), a0);
      if (k + 1 < Ta) a1 = __fmaf_rn(taps[k + 1], d(k + 1), a1);
      if (k + 2 < Ta) a2 = __fmaf_rn(taps[k + 2], d(k + 2), a2);
      out[j * K + s] = __fadd_rn(__fadd_rn(a0, a1), __fadd_rn(a2, a3));
    }
    __syncthreads();  // the next tile overwrites the column
  }
}

__global__ void demod_mode_kernel(uint2 *par, int s_first, int s_count, uint32_t mode, uint32_t word) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < s_count) par[s_first + i] = uint2{mode, word};
}

}  // namespace

hipError_t launch_demod_push(const float2 *x, int64_t steps, int64_t step_stride, int64_t stream_stride, uint64_t n0,
                             int K, int Ta, int Da, const DemodForm &f, const DemodCut &c, const float *taps,
                             const uint32_t *par, const float2 *carry_old, float2 *carry_new, float *out,
                             hipStream_t st) {
  int ll = 0;
  while ((1 << ll) < f.lanes) ++ll;
  if (!f.ok() || !c.ok() || f.lds_bytes > kDemodLdsMax || (1 << ll) != f.lanes || f.lanes > kDemodLanesMax ||
      (f.kind == kDemodTime) != (f.lanes == 1) || f.halo != Ta - 1 || f.span != f.outs * Da ||
      f.lds_bytes < 4 * f.lanes * (demod_row(f.halo + f.span - 1, f.kind) + 1) ||
      f.stream_tiles != (K + f.lanes - 1) / f.lanes || c.nspans != (steps + f.span - 1) / f.span ||
      c.ntiles != c.nspans * f.stream_tiles || c.r0 < 0 || c.r0 >= Da || !demod_strides_ok(K, step_stride, stream_stride))
    return hipErrorInvalidValue;
  const DemodGeom g{steps, c.nspans, c.ntiles, step_stride, stream_stride, (uint32_t)n0, K, Ta, Da, c.r0,
                    ll, f.span, f.halo, f.stream_tiles};
  const dim3 grid((unsigned)c.grid), block(kDemodThreads);
  const v2f *xv = (const v2f *)x, *co = (const v2f *)carry_old;
  v2f *cn = (v2f *)carry_new;
  const uint2 *pp = (const uint2 *)par;
  if (f.kind == kDemodTime)
    demod_push_kernel<kDemodTime><<<grid, block, f.lds_bytes, st>>>(xv, g, taps, pp, co, cn, out);
  else
    demod_push_kernel<kDemodStreams><<<grid, block, f.lds_bytes, st>>>(xv, g, taps, pp, co, cn, out);
  return hipGetLastError();
}

hipError_t launch_demod_mode(uint32_t *par, int s_first, int s_count, uint32_t mode, uint32_t word, hipStream_t st) {
  if (s_first < 0 || s_count < 1 || s_first + s_count > kDemodMaxStreams || mode > ZFFT_DEMOD_POWER)
    return hipErrorInvalidValue;
  demod_mode_kernel<<<dim3((unsigned)((s_count + 255) / 256)), dim3(256), 0, st>>>((uint2 *)par, s_first, s_count, mode, word);
  return hipGetLastError();
}

}  // namespace zfft
