// chan_kernels.hip -- the channeliser's push (rule: zfft.h, zfft_plan_chan; form: zfft_chan_plan.h;
// DESIGN §3.3.10).  One launch per push: a workgroup takes spans of whole steps round-robin, stages
// a span in LDS as complex64 behind the M P - 1 samples before it (from the carry where those
// precede the push), writes its part of the next carry, and turns the span's steps into channels.
//
// Pass 1 is the polyphase FIR and the first butterfly of the transform in one: lane j < M / R1 of
// a step holds the branches s = j + r M / R1, r < R1 -- the inputs of one radix-R1 butterfly of a
// decimation-in-frequency FFT -- so consecutive lanes read consecutive samples, and the branch
// sums never go through LDS.  A lane's j is the same for every step it takes, so its R1 P
// coefficients are loaded once per workgroup: into registers for P <= 8 (kChanRegs: one kernel per
// P, so the sums unroll), into LDS otherwise (kChanLds).  With D = M / 2 the odd steps need the coefficient set half a turn on,
// which for these lanes is the same set under r -> r + R1 / 2: one set serves both.
//
// The remaining passes are radix 4 in place in LDS (one barrier each, no second buffer); the
// result is in digit-reversed order, which the store undoes through a small table of the kept
// channels' positions, so a wave writes contiguous runs of out[step][kept channel].
//
// Order of operations (what makes the outputs independent of how the stream is cut): a branch
// is P fused multiply-adds per component from zero in ascending k; the transform is a fixed
// function of M.  Nothing depends on the span, the lane or the push.
#include <hip/hip_runtime.h>

#include "zfft_device.h"
#include "zfft_fft.h"
#include "zfft_chan_plan.h"

namespace zfft {
namespace {

struct ChanGeom {
  int64_t n, steps, nspans;  // samples, steps and spans of the push
  int span, S, points, halo; // ChanForm's (S = steps_per_span)
  int M, P, D;
  int r0, odd0;
  int c_first, K;
  int dtype;
};

// chan_position (zfft_chan_plan.h) for a first radix R1
template <int R1>
__device__ __forceinline__ int chan_pos(int M, int c) {
  int L = M / R1, pos = (c % R1) * L;
  c /= R1;
  while (L > 1) {
    L >>= 2;
    pos += (c & 3) * L;
    c >>= 2;
  }
  return pos;
}

// A span's samples and the halo before them into xs, and the span's part of the next carry.
template <int DT>
__device__ __forceinline__ void chan_stage_t(const void *in, const ChanGeom &g, int64_t b, v2f *xs,
                                             const v2f *carry_old, v2f *carry_new) {
  const int H = g.halo;
  const InDesc d{in, g.n, g.n, DT, 0};
  const int64_t s0 = b * g.span, s1 = s0 + g.span < g.n ? s0 + g.span : g.n;
  const int count = H + (int)(s1 - s0);
  const int64_t keep0 = g.n - H;
  for (int i = threadIdx.x; i < count; i += kChanThreads) {
    const int64_t r = s0 - H + i;
    const v2f v = r < 0 ? carry_old[H + r] : load_in_t<DT, 0>(d, 0, r);
    xs[i] = v;
    if (i >= H && r >= keep0) carry_new[r - keep0] = v;
  }
}

__device__ __forceinline__ void chan_stage(const void *in, const ChanGeom &g, int64_t b, v2f *xs, const v2f *carry_old,
                                           v2f *carry_new) {
  switch (g.dtype) {
    case kInC64: chan_stage_t<kInC64>(in, g, b, xs, carry_old, carry_new); break;
    case kInC32H: chan_stage_t<kInC32H>(in, g, b, xs, carry_old, carry_new); break;
    case kInCU8: chan_stage_t<kInCU8>(in, g, b, xs, carry_old, carry_new); break;
    default: chan_stage_t<kInF32R>(in, g, b, xs, carry_old, carry_new); break;
  }
}

// PT: the taps per branch where they are known at compile time (kChanRegs), else 0 (kChanLds)
template <int R1, int PT>
__global__ void __launch_bounds__(kChanThreads) chan_push_kernel(const void *__restrict__ in, ChanGeom g,
                                                                const float *__restrict__ h,
                                                                const v2f *__restrict__ tw,
                                                                const v2f *__restrict__ carry_old,
                                                                v2f *__restrict__ carry_new,
                                                                v2f *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) v2f lds[];
  const int tid = threadIdx.x, M = g.M, P = g.P, D = g.D, H = g.halo, S = g.S, K = g.K;
  v2f *fb = lds, *tws = fb + g.points, *xs = tws + M;  // the transform, W_M^i, the staging
  int *perm = (int *)(xs + H + g.span);                // where kept channel i ends in a step's M points
  float *hs = (float *)(perm + K);                     // the prototype (kChanLds)
  const int Q = M / R1, logQ = __ffs(Q) - 1, logM4 = __ffs(M) - 3;
  const int j = tid & (Q - 1), sub = tid >> logQ, spi = kChanThreads >> logQ;

  for (int i = tid; i < M; i += kChanThreads) tws[i] = tw[i];
  for (int i = tid; i < K; i += kChanThreads) perm[i] = chan_pos<R1>(M, (g.c_first + i) & (M - 1));
  if (PT == 0)
    for (int i = tid; i < M * P; i += kChanThreads) hs[i] = h[i];
  // branch s = j + r Q of an even step sums h[k0 + p M] x[m D - k0 - p M], k0 = -s mod M
  int k0[R1];
  float c[R1][PT ? PT : 1];
#pragma unroll
  for (int r = 0; r < R1; ++r) {
    k0[r] = (-(j + r * Q)) & (M - 1);
#pragma unroll
    for (int p = 0; p < PT; ++p) c[r][p] = h[k0[r] + p * M];
  }

  const int64_t keep0 = g.n - H;  // the next carry holds the samples from here on
  for (int64_t b = blockIdx.x; b < g.nspans; b += gridDim.x) {
    chan_stage(in, g, b, xs, carry_old, carry_new);
    // a push shorter than the carry: the rest of it is the old one's end
    if (b == 0)
      for (int64_t i = tid; i < -keep0; i += kChanThreads) carry_new[i] = carry_old[i + g.n];
    __syncthreads();

    // pass 1: the branch sums of a butterfly, the butterfly, its twiddles W_M^(j r)
    const int64_t jb0 = b * S;  // the span's first step, counted in the push
    for (int l = sub; l < S; l += spi) {
      // (a step past the push's last, in the last span, sums stale staging: it is never stored)
      v2f u[R1];
      const int i0 = H + g.r0 + l * D;  // x[m D] in the staging; i0 - k >= 0 for k < M P
#pragma unroll
      for (int r = 0; r < R1; ++r) {
        v2f a = splat(0.f);
        const v2f *x = xs + i0 - k0[r];
        if (PT) {
#pragma unroll
          for (int p = 0; p < PT; ++p) a = vfma(splat(c[r][p]), x[-p * M], a);
        } else {
          const float *hh = hs + k0[r];
          for (int p = 0; p < P; ++p) a = vfma(splat(hh[p * M]), x[-p * M], a);
        }
        u[r] = a;
      }
      // an odd step at D = M / 2: the sums are those of the branches half a turn on
      const bool odd = D != M && ((g.odd0 + jb0 + l) & 1);
      v2f v[R1];
#pragma unroll
      for (int r = 0; r < R1; ++r) v[r] = odd ? u[(r + R1 / 2) % R1] : u[r];
      dft<R1>(v);
      v2f *o = fb + l * M + j;
      o[0] = v[0];
#pragma unroll
      for (int r = 1; r < R1; ++r) o[r * Q] = Q > 1 ? cmul2(v[r], tws[j * r]) : v[r];
    }
    __syncthreads();

    // the radix-4 passes on the lengths L = Q, Q / 4, ..., 4, every step of the span at once
    for (int L = Q; L >= 4; L >>= 2) {
      const int Lq = L >> 2, scale = M / L, items = S << logM4;
      for (int it = tid; it < items; it += kChanThreads) {
        const int l = it >> logM4, jj = it & ((M >> 2) - 1), q = jj & (Lq - 1);
        v2f *e = fb + l * M + ((jj - q) << 2) + q;
        v2f v[4] = {e[0], e[Lq], e[2 * Lq], e[3 * Lq]};
        dft<4>(v);
        e[0] = v[0];
#pragma unroll
        for (int r = 1; r < 4; ++r) e[r * Lq] = L > 4 ? cmul2(v[r], tws[q * r * scale]) : v[r];
      }
      __syncthreads();
    }

    // out[step][kept channel]: consecutive threads, consecutive addresses
    const int64_t left = g.steps - jb0;
    const int items = (int)(left < S ? (left > 0 ? left : 0) : S) * K;
    v2f *o = out + jb0 * K;
    int l = tid / K, i = tid - l * K;
    const int dl = kChanThreads / K, di = kChanThreads - dl * K;
    for (int it = tid; it < items; it += kChanThreads) {
      o[it] = fb[l * M + perm[i]];
      l += dl, i += di;
      if (i >= K) i -= K, ++l;
    }
  }
}

}  // namespace

hipError_t launch_chan_push(const void *in, int dtype, int64_t n, int M, int P, int D, int c_first, int K,
                            const ChanForm &f, const float *h, const float2 *tw, const float2 *carry_old,
                            float2 *carry_new, float2 *out, hipStream_t st) {
  if (!f.ok() || f.grid < 1 || f.lds_bytes > kChanLdsMax || (f.radix1 != 4 && f.radix1 != 8) ||
      f.halo != M * P - 1 || f.span != f.steps_per_span * D || f.points != f.steps_per_span * M ||
      dtype < kInC64 || dtype > kInF32R || c_first < 0 || c_first >= M || K < 1 || K > M)
    return hipErrorInvalidValue;
  const ChanGeom g{n, f.steps, f.nspans, f.span, f.steps_per_span, f.points, f.halo, M, P, D,
                   f.r0, f.odd0, c_first, K, dtype};
  const dim3 grid((unsigned)f.grid), block(kChanThreads);
  const v2f *t = (const v2f *)tw, *co = (const v2f *)carry_old;
  v2f *cn = (v2f *)carry_new, *o = (v2f *)out;
  using Kernel = void (*)(const void *, ChanGeom, const float *, const v2f *, const v2f *, v2f *, v2f *);
#define ZFFT_CHAN_ROW(R) \
  {chan_push_kernel<R, 0>, chan_push_kernel<R, 1>, chan_push_kernel<R, 2>, chan_push_kernel<R, 3>, chan_push_kernel<R, 4>, \
   chan_push_kernel<R, 5>, chan_push_kernel<R, 6>, chan_push_kernel<R, 7>, chan_push_kernel<R, 8>}
  static const Kernel kernels[2][kChanRegTaps + 1] = {ZFFT_CHAN_ROW(4), ZFFT_CHAN_ROW(8)};
#undef ZFFT_CHAN_ROW
  static_assert(kChanRegTaps == 8, "one kernel per P up to kChanRegTaps");
  if ((f.kind == kChanRegs) != (P <= kChanRegTaps)) return hipErrorInvalidValue;
  kernels[f.radix1 == 8][f.kind == kChanRegs ? P : 0]<<<grid, block, f.lds_bytes, st>>>(in, g, h, t, co, cn, o);
  return hipGetLastError();
}

}  // namespace zfft
