// tap_kernels.hip -- the channel taps' push (rule: zfft.h, zfft_plan_taps; form: zfft_tap_plan.h;
// DESIGN §3.3.9).  One launch serves every open tap: a workgroup owns a span of the push's input,
// stages it in LDS as complex64 behind the `halo` samples before it (from the carry where those
// precede the push), writes its part of the next carry, and walks the open taps over the span.
//
// Mapping: a wave takes 64 consecutive outputs of one tap (a chunk), one output per lane; the
// chunks of all taps go round the four waves.  A lane's reads are D samples from its neighbour's,
// so the staging pads one slot per 2^pad_shift, the shift chosen per push for the open taps
// (tap_slot, choose_tap); the table c[k] is the same for the whole wave and is read through
// wave-uniform addresses into scalar registers.
//
// Summation order (what makes the outputs independent of how the stream is cut): four partial
// sums, a_j over the k = j (mod 4) in ascending k, each step the two fused multiply-adds of
// cmac2; then y = rot * ((a_0 + a_1) + (a_2 + a_3)).  Nothing in it depends on the span, the
// lane or the push.
#include <hip/hip_runtime.h>

#include "zfft_device.h"
#include "zfft_tap_plan.h"

namespace zfft {
namespace {

// acc + c x (complex) in two VOP3P instructions, as fc_kernels.hip's cmac2; c in scalar registers
__device__ __forceinline__ v2f cmac2s(v2f acc, v2f c, v2f x) {
  v2f t, r;
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1]" : "=v"(t) : "s"(c), "v"(x), "v"(acc));
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]"
      : "=v"(r) : "s"(c), "v"(x), "v"(t));
  return r;
}

// exp(-2 pi i ph / 2^32): the high 24 bits are an exact float argument of sincospi, the low 8 a
// small angle d <= 2 pi 2^-24 (cos d = 1 to 7e-14, sin d = d)
__device__ __forceinline__ v2f tap_rot(uint32_t ph) {
  float s, c;
  sincospif((float)(ph >> 8) * 0x1p-23f, &s, &c);
  const float d = (float)(ph & 255u) * (float)(6.283185307179586 / 4294967296.0);
  return v2f{fmaf(-d, s, c), -fmaf(d, c, s)};
}

struct TapGeom {
  int64_t n;       // samples of the push
  int span, halo;  // TapForm's
  int pad_shift;
  int H;           // max_len - 1: the carry's length
  int max_len;     // the table's row stride
  int first_span, ntaps;
};

template <int DT>
__global__ void __launch_bounds__(kTapThreads) tap_push_kernel(const void *__restrict__ in, TapGeom g,
                                                              const v2f *__restrict__ tab,
                                                              const v2f *__restrict__ carry_old,
                                                              v2f *__restrict__ carry_new, v2f *__restrict__ out,
                                                              TapItems items) {
  extern __shared__ __attribute__((aligned(16))) v2f xs[];
  const int tid = threadIdx.x;
  const int64_t b = (int64_t)blockIdx.x + g.first_span;
  const int64_t s0 = b * g.span, s1 = s0 + g.span < g.n ? s0 + g.span : g.n;
  const int len = (int)(s1 - s0), halo = g.halo, sh = g.pad_shift;
  const int64_t keep0 = g.n - g.H;  // the next carry holds the samples from here on
  const InDesc d{in, g.n, g.n, DT, 0};
  for (int i = tid; i < halo + len; i += kTapThreads) {
    const int64_t r = s0 - halo + i;  // >= -halo >= -H
    const v2f v = r < 0 ? carry_old[g.H + r] : load_in_t<DT, 0>(d, 0, r);
    xs[tap_slot(i, sh)] = v;
    if (i >= halo && r >= keep0) carry_new[r - keep0] = v;
  }
  // a push shorter than the carry: the rest of it is the old one's end
  if (b == 0)
    for (int64_t j = tid; j < -keep0; j += kTapThreads) carry_new[j] = carry_old[j + g.n];
  __syncthreads();

  const int wave = tid >> 6, lane = tid & 63;
  int turn = 0;  // chunks given out so far (mod 4): the next goes to wave `turn`
  for (int ti = 0; ti < g.ntaps; ++ti) {
    const TapItem &t = items.t[ti];
    const int D = t.D, T = t.T;
    // the outputs j with s0 <= r0 + j D < s1
    const int64_t d0 = s0 - t.r0, d1 = s1 - t.r0;
    const int64_t j0 = d0 <= 0 ? 0 : (d0 + D - 1) / D, j1 = d1 <= 0 ? 0 : (d1 + D - 1) / D;
    const int cnt = (int)(j1 - j0), chunks = (cnt + 63) >> 6;
    const v2f *c = tab + (size_t)t.slot * g.max_len;
    for (int ch = (wave - turn) & 3; ch < chunks; ch += 4) {
      const int jj = ch * 64 + lane;
      if (jj < cnt) {
        const int64_t j = j0 + jj;
        const int i0 = (int)(t.r0 + j * D - s0) + halo;  // x[m D] in the staging; i0 - k >= 0 for k < T
        v2f a0 = splat(0.f), a1 = a0, a2 = a0, a3 = a0;
        int k = 0;
        auto mac4 = [&](int q) {
          a0 = cmac2s(a0, c[q], xs[tap_slot(i0 - q, sh)]);
          a1 = cmac2s(a1, c[q + 1], xs[tap_slot(i0 - q - 1, sh)]);
          a2 = cmac2s(a2, c[q + 2], xs[tap_slot(i0 - q - 2, sh)]);
          a3 = cmac2s(a3, c[q + 3], xs[tap_slot(i0 - q - 3, sh)]);
        };
        for (; k + 16 <= T; k += 16) {  // (the same order, sixteen table entries and reads in flight)
          mac4(k);
          mac4(k + 4);
          mac4(k + 8);
          mac4(k + 12);
        }
        for (; k + 4 <= T; k += 4) mac4(k);
        if (k < T) a0 = cmac2s(a0, c[k], xs[tap_slot(i0 - k, sh)]);
        if (k + 1 < T) a1 = cmac2s(a1, c[k + 1], xs[tap_slot(i0 - k - 1, sh)]);
        if (k + 2 < T) a2 = cmac2s(a2, c[k + 2], xs[tap_slot(i0 - k - 2, sh)]);
        const v2f y = (a0 + a1) + (a2 + a3);
        out[t.out_off + j] = cmul2(tap_rot(t.ph0 + (uint32_t)j * t.dph), y);
      }
    }
    turn = (turn + chunks) & 3;
  }
}

}  // namespace

hipError_t launch_tap_push(const void *in, int dtype, int64_t n, int max_len, const TapForm &f, const TapItems &items,
                           const float2 *tab, const float2 *carry_old, float2 *carry_new, float2 *out,
                           hipStream_t st) {
  if (!f.ok() || f.grid < 1 || f.lds_bytes > kTapLdsMax) return hipErrorInvalidValue;
  const TapGeom g{n, f.span, f.halo, f.pad_shift, max_len - 1, max_len, f.first_span, f.ntaps};
  const dim3 grid((unsigned)f.grid), block(kTapThreads);
  const v2f *t = (const v2f *)tab, *co = (const v2f *)carry_old;
  v2f *cn = (v2f *)carry_new, *o = (v2f *)out;
  switch (dtype) {
    case kInC64: tap_push_kernel<kInC64><<<grid, block, f.lds_bytes, st>>>(in, g, t, co, cn, o, items); break;
    case kInC32H: tap_push_kernel<kInC32H><<<grid, block, f.lds_bytes, st>>>(in, g, t, co, cn, o, items); break;
    case kInCU8: tap_push_kernel<kInCU8><<<grid, block, f.lds_bytes, st>>>(in, g, t, co, cn, o, items); break;
    case kInF32R: tap_push_kernel<kInF32R><<<grid, block, f.lds_bytes, st>>>(in, g, t, co, cn, o, items); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace zfft
