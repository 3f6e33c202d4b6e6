// history_kernels.hip -- the row history of libzfft.so: pushed rows kept on the device as a ring
// of float32 rows or of 16- / 8-bit codes on a fixed level scale, and re-reduced to any window,
// time scale and detector (rule: zfft.h, zfft_plan_history; entry points: zfft_history.cpp;
// quantiser and form chooser: zfft_history_plan.h).  A file of its own, so the
// code objects of the other kernel files stay as they were.
//
// The store.  Row R lives in slot R mod cap, `stride` = n rounded up to 16 elements per slot:
// every slot starts on a 16-byte boundary in every format, and an aligned 16-byte load that
// begins inside a slot ends inside it.  The elements at or beyond n are padding (code 0 / NaN).
//
// history_pack_kernel / history_unpack_kernel.  A thread owns four consecutive columns of a run
// of rows: one 16-byte load of floats (four scalar loads when the caller's rows are not 16-byte
// aligned, n_win no multiple of 4) and one 4-, 8- or 16-byte store of codes, and the reverse.
//
// history_view_kernel<format, detector>.  A workgroup of four waves owns one column tile -- px
// consecutive pixels -- and a run of lines (or, in the sliced form, one slice of one line's
// rows).  The tile's columns start at ca, the 16-byte boundary at or below the first bucket's
// edge; lane l of a wave loads the 16 bytes of columns ca + l E ... of a row (E = 16, 8 or 4
// columns), four rows in flight per wave, the rows of a line dealt to the four waves.  MAX and
// MIN reduce in the code domain: four U8 codes of a dword widen to two packed-u16 words, so one
// packed 16-bit max / min takes two codes; MIN compares code - 1 (packed, wrapping), which makes
// the NaN code 0 the largest value, and an all-NaN cell wraps back to code 0 at the end.  Columns
// outside the tile's buckets (the unaligned head, the tail, the padding) are masked to the
// identity as they are loaded, so a bucket wider than a wave's columns folds further blocks of
// columns onto the same accumulators (px = 1).  MEAN adds 10^(v'/20) of the unpacked value, from
// a 256-entry table in LDS for U8: four rows in float32, every further sum in float64.  The waves
// meet in LDS in one column-resolution reduced row, pixel threads reduce their buckets from it
// and unpack once.  A line with a row outside [oldest, seen) is written as NaN and loads nothing.
// history_finish_kernel combines a sliced view's partials per pixel.
// No workgroup waits for another and there is no atomic.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "zfft_internal.h"

namespace zfft {

namespace {

constexpr int kU = 4;  // rows a wave loads at once
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned pack_code(const HistQuant &q, float v) {
  if (v != v) return 0u;
  const float t = __fmul_rn(__fsub_rn(v, q.lo), q.inv);  // two roundings
  return 1u + (unsigned)(int)rintf(fminf(fmaxf(t, 0.f), (float)q.K));
}

__device__ __forceinline__ float unpack_code(const HistQuant &q, unsigned code) {
#pragma clang fp contract(off)
  const float prod = (float)((int)code - 1) * q.step;  // (both written here, under the pragma: the
  const float v = q.lo + prod;                         // header's __fmul_rn is a plain, fusable product)
  return code == 0u ? __builtin_nanf("") : v;
}

__device__ __forceinline__ float lin_amp(float v) { return exp2f(v * 0.16609640474436813f); }  // 10^(v/20)

template <int FMT>
struct Fmt {
  static constexpr int EB = FMT == kHistF32 ? 4 : FMT == kHistU16 ? 2 : 1;
  static constexpr int E = kHistLaneBytes / EB, T = 64 * E;
};

// ------------------------------------------------------------------ pack / unpack
template <int FMT>
__global__ __launch_bounds__(256) void history_pack_kernel(const float *__restrict__ rows, int n_win, int count,
                                                            int64_t slot0, HistStore s, int vec) {
  const int c = 4 * (blockIdx.x * 256 + threadIdx.x);
  if (c >= s.stride) return;
  for (int i = blockIdx.y; i < count; i += gridDim.y) {
    const float *pr = rows + (int64_t)i * n_win + c;
    float v[4];
    if (vec && c + 3 < s.n) {
      const float4 q = *reinterpret_cast<const float4 *>(pr);
      v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = c + e < s.n ? pr[e] : __builtin_nanf("");
    }
    const int64_t slot = slot0 + i;  // (count <= cap: at most one wrap)
    const int64_t at = (slot >= s.cap ? slot - s.cap : slot) * s.stride + c;
    if constexpr (FMT == kHistF32) {
      *reinterpret_cast<float4 *>(static_cast<float *>(s.data) + at) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      unsigned k[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) k[e] = c + e < s.n ? pack_code(s.q, v[e]) : 0u;
      if constexpr (FMT == kHistU16)
        *reinterpret_cast<uint2 *>(static_cast<uint16_t *>(s.data) + at) = make_uint2(k[0] | k[1] << 16, k[2] | k[3] << 16);
      else
        *reinterpret_cast<unsigned *>(static_cast<uint8_t *>(s.data) + at) = k[0] | k[1] << 8 | k[2] << 16 | k[3] << 24;
    }
  }
}

template <int FMT>
__global__ __launch_bounds__(256) void history_unpack_kernel(HistStore s, int64_t slot0, int count, int n_win,
                                                              float *__restrict__ rows, int vec) {
  const int c = 4 * (blockIdx.x * 256 + threadIdx.x);
  if (c >= s.n) return;
  for (int i = blockIdx.y; i < count; i += gridDim.y) {
    const int64_t slot = slot0 + i;  // (count <= cap: at most one wrap)
    const int64_t at = (slot >= s.cap ? slot - s.cap : slot) * s.stride + c;
    float v[4];
    if constexpr (FMT == kHistF32) {
      const float4 q = *reinterpret_cast<const float4 *>(static_cast<const float *>(s.data) + at);
      v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else if constexpr (FMT == kHistU16) {
      const uint2 q = *reinterpret_cast<const uint2 *>(static_cast<const uint16_t *>(s.data) + at);
      v[0] = unpack_code(s.q, q.x & 0xffffu), v[1] = unpack_code(s.q, q.x >> 16);
      v[2] = unpack_code(s.q, q.y & 0xffffu), v[3] = unpack_code(s.q, q.y >> 16);
    } else {
      const unsigned q = *reinterpret_cast<const unsigned *>(static_cast<const uint8_t *>(s.data) + at);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = unpack_code(s.q, (q >> (8 * e)) & 0xffu);
    }
    float *pr = rows + (int64_t)i * n_win + c;
    if (vec && c + 3 < s.n) {
      *reinterpret_cast<float4 *>(pr) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c + e < s.n) pr[e] = v[e];
    }
  }
}

// ------------------------------------------------------------------ view
// What a column, a bucket and a slice are reduced in: codes (MAX: the code; MIN: code - 1 modulo
// 2^16), float32 values (F32 MAX / MIN) or float64 linear sums (MEAN).
template <int FMT, int DET>
struct HRed {
  using C = std::conditional_t<DET == 2, double, std::conditional_t<FMT == kHistF32, float, unsigned>>;
  static __device__ __forceinline__ C ident() {
    if constexpr (DET == 2)
      return 0.0;
    else if constexpr (FMT == kHistF32)
      return __builtin_nanf("");
    else
      return DET == 0 ? 0u : 0xffffu;
  }
  static __device__ __forceinline__ C comb(C a, C b) {
    if constexpr (DET == 2)
      return a + b;
    else if constexpr (FMT == kHistF32)
      return DET == 0 ? fmaxf(a, b) : fminf(a, b);
    else
      return DET == 0 ? max(a, b) : min(a, b);
  }
  static __device__ __forceinline__ float fin(C a, double cells, const HistQuant &q) {
    if constexpr (DET == 2)
      return (float)(20.0 * log10(a / cells));
    else if constexpr (FMT == kHistF32)
      return a;
    else
      return unpack_code(q, DET == 0 ? a : ((a + 1u) & 0xffffu));
  }
};

__device__ __forceinline__ int hedge(const HistGeom &g, int x) {
  return g.col0 + (int)((int64_t)x * g.span / g.width);
}
__device__ __forceinline__ bool line_in_store(const HistGeom &g, int j) {
  const int64_t r0 = g.first + (int64_t)j * g.m;
  return r0 >= g.oldest && r0 + g.m <= g.seen;
}
__device__ __forceinline__ u16x2 as_pk(unsigned d) { return __builtin_bit_cast(u16x2, d); }
__device__ __forceinline__ unsigned dword(const uint4 &v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }

template <int FMT, int DET>
__global__ __launch_bounds__(64 * kHistWaves) void history_view_kernel(HistStore s, HistGeom g, HistForm f,
                                                                        float *__restrict__ img,
                                                                        void *__restrict__ scratch) {
  using R = HRed<FMT, DET>;
  using C = typename R::C;
  constexpr int EB = Fmt<FMT>::EB, E = Fmt<FMT>::E, T = Fmt<FMT>::T;
  constexpr bool kCodes = FMT != kHistF32 && DET != 2;
  constexpr bool kTable = FMT == kHistU8 && DET == 2;
  constexpr int NA = kCodes ? (FMT == kHistU8 ? 8 : 4) : E;  // accumulators per lane
  using A = std::conditional_t<kCodes, u16x2, C>;
  __shared__ C lds[kHistWaves][T];
  __shared__ C wred[kHistWaves];
  __shared__ float tab[kTable ? 256 : 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if constexpr (kTable) {
    tab[tid] = (tid >= 1 && tid <= s.q.K + 1) ? lin_amp(unpack_code(s.q, (unsigned)tid)) : __builtin_nanf("");
    __syncthreads();
  }
  const int x0 = blockIdx.y * f.px, x1 = min(g.width, x0 + f.px), npx = x1 - x0;
  const int c0 = hedge(g, x0), c1 = hedge(g, x1);
  const int ca = c0 & ~(E - 1);
  const bool folded = c1 - ca > T;  // (then px = 1: every column is pixel x0's)
  const bool sliced = f.kind == kHistSliced;
  const int j0 = sliced ? (int)blockIdx.x / f.s : (int)min((int64_t)blockIdx.x * f.k, (int64_t)g.lines);
  const int j1 = sliced ? j0 + 1 : (int)min((int64_t)j0 + f.k, (int64_t)g.lines);
  const int kk = sliced ? (int)blockIdx.x % f.s : 0;
  const uint8_t *base = static_cast<const uint8_t *>(s.data);
  C *part = static_cast<C *>(scratch);

  for (int j = j0; j < j1; ++j) {
    if (!line_in_store(g, j)) {  // (uniform) the finishing launch writes a sliced view's NaN lines
      if (!sliced)
        for (int p = tid; p < npx; p += 64 * kHistWaves) img[(int64_t)j * g.width + x0 + p] = __builtin_nanf("");
      continue;
    }
    const int ia = sliced ? kk * f.slice_rows : 0, ib = sliced ? min(g.m, ia + f.slice_rows) : g.m;
    const int64_t s0 = (g.first + (int64_t)j * g.m) % s.cap;  // the line's first slot; its rows are in the store
    A acc[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      if constexpr (kCodes)
        acc[a] = as_pk(DET == 0 ? 0u : 0xffffffffu);
      else
        acc[a] = R::ident();
    }
    for (int cb = ca; cb < c1; cb += T) {
      const int col = cb + lane * E;  // the lane's first column: a 16-byte boundary inside the slot
      const bool live = col < c1;
      // the bytes of the lane's 16 that lie in [c0, c1): one run [ba, bb), cut into its dwords
      const int ba = EB * min(max(c0 - col, 0), E), bb = EB * min(max(c1 - col, 0), E);
      unsigned mw[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int a = min(max(ba - 4 * k, 0), 4), b = min(max(bb - 4 * k, 0), 4);
        mw[k] = b > a ? (unsigned)(((1ull << (8 * b)) - 1ull) ^ ((1ull << (8 * a)) - 1ull)) : 0u;
      }
      for (int i = ia + wave * kU; i < ib; i += kHistWaves * kU) {
        // rows past the line's (slice's) end repeat its last row: harmless to max / min, masked by MEAN
        uint4 v[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          int64_t slot = s0 + min(i + u, ib - 1);
          if (slot >= s.cap) slot -= s.cap;
          v[u] = make_uint4(0u, 0u, 0u, 0u);
          if (live) v[u] = *reinterpret_cast<const uint4 *>(base + (slot * s.stride + col) * EB);
        }
        if constexpr (kCodes) {
#pragma unroll
          for (int u = 0; u < kU; ++u) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const unsigned d = dword(v[u], k) & mw[k];
              if constexpr (FMT == kHistU8) {
                u16x2 lo = as_pk(d & 0x00ff00ffu), hi = as_pk((d >> 8) & 0x00ff00ffu);  // columns 4k, 4k+2 / 4k+1, 4k+3
                if constexpr (DET == 1) lo -= u16x2{1, 1}, hi -= u16x2{1, 1};
                acc[2 * k] = DET == 0 ? __builtin_elementwise_max(acc[2 * k], lo) : __builtin_elementwise_min(acc[2 * k], lo);
                acc[2 * k + 1] = DET == 0 ? __builtin_elementwise_max(acc[2 * k + 1], hi) : __builtin_elementwise_min(acc[2 * k + 1], hi);
              } else {
                u16x2 w = as_pk(d);  // columns 2k, 2k+1
                if constexpr (DET == 1) w -= u16x2{1, 1};
                acc[k] = DET == 0 ? __builtin_elementwise_max(acc[k], w) : __builtin_elementwise_min(acc[k], w);
              }
            }
          }
        } else if constexpr (DET != 2) {  // float32 rows: a masked column is NaN, the identity
#pragma unroll
          for (int u = 0; u < kU; ++u) {
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = R::comb(acc[k], __uint_as_float(dword(v[u], k) | ~mw[k]));
          }
        } else {
#pragma unroll
          for (int e = 0; e < E; ++e) {
            float sum = 0.f;
#pragma unroll
            for (int u = 0; u < kU; ++u) {
              const unsigned d = dword(v[u], e * EB / 4);
              float t;
              if constexpr (FMT == kHistF32)
                t = lin_amp(__uint_as_float(d));
              else if constexpr (FMT == kHistU16)
                t = lin_amp(unpack_code(s.q, (d >> (16 * (e & 1))) & 0xffffu));  // (code 0: NaN through exp2f)
              else
                t = tab[(d >> (8 * (e & 3))) & 0xffu];
              sum += i + u < ib ? t : 0.f;
            }
            const bool ok = (mw[e * EB / 4] >> (8 * (e * EB % 4))) & 1u;
            acc[e] += ok ? (double)sum : 0.0;
          }
        }
      }
    }
    // ---- one column-resolution reduced row: the waves' rows, then their combination in lds[0]
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      if constexpr (kCodes && FMT == kHistU8) {
        const int k = a >> 1, odd = a & 1;
        lds[wave][lane * E + 4 * k + odd] = acc[a].x;
        lds[wave][lane * E + 4 * k + odd + 2] = acc[a].y;
      } else if constexpr (kCodes) {
        lds[wave][lane * E + 2 * a] = acc[a].x;
        lds[wave][lane * E + 2 * a + 1] = acc[a].y;
      } else {
        lds[wave][lane * E + a] = acc[a];
      }
    }
    __syncthreads();
    C mine = R::ident();
    for (int c = tid; c < T; c += 64 * kHistWaves) {
      const C a = R::comb(R::comb(lds[0][c], lds[1][c]), R::comb(lds[2][c], lds[3][c]));
      lds[0][c] = a;  // (column c is this thread's alone)
      mine = R::comb(mine, a);
    }
    if (folded) {
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) mine = R::comb(mine, __shfl_xor(mine, d));
      if (lane == 0) wred[wave] = mine;
    }
    __syncthreads();
    // ---- buckets, then where the value goes
    for (int p = tid; p < npx; p += 64 * kHistWaves) {
      const int x = x0 + p, e0 = hedge(g, x), e1 = hedge(g, x + 1);
      C a = R::ident();
      if (folded) {
        a = R::comb(R::comb(wred[0], wred[1]), R::comb(wred[2], wred[3]));
      } else {
        for (int c = e0 - ca; c < e1 - ca; ++c) a = R::comb(a, lds[0][c]);
      }
      if (sliced)
        part[((int64_t)j * f.s + kk) * g.width + x] = a;
      else
        img[(int64_t)j * g.width + x] = R::fin(a, (double)g.m * (double)(e1 - e0), s.q);
    }
    __syncthreads();  // lds is the next line's
  }
}

template <int FMT, int DET>
__global__ __launch_bounds__(256) void history_finish_kernel(HistStore s, HistGeom g, HistForm f, float *__restrict__ img,
                                                              const void *__restrict__ scratch) {
  using R = HRed<FMT, DET>;
  using C = typename R::C;
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= (int64_t)g.lines * g.width) return;
  const int j = (int)(id / g.width), x = (int)(id % g.width);
  if (!line_in_store(g, j)) {
    img[id] = __builtin_nanf("");
    return;
  }
  const C *pj = static_cast<const C *>(scratch) + (int64_t)j * f.s * g.width + x;
  C a = R::ident();
  for (int k = 0; k < f.s; ++k) a = R::comb(a, pj[(int64_t)k * g.width]);
  img[id] = R::fin(a, (double)g.m * (double)(hedge(g, x + 1) - hedge(g, x)), s.q);
}

bool store_ok(const HistStore &s) {
  return s.data && s.cap >= 1 && s.n >= 1 && s.stride == hist_stride(s.n) && hist_format_ok(s.q.format) &&
         (s.q.format == kHistF32 || s.q.K == (s.q.format == kHistU8 ? 254 : 65534));
}

// The form must be choose_history's for this window (recomputed here: the grid and the scratch
// layout follow from it), the window inside a stored row, the scratch large enough.
bool view_ok(const HistStore &s, const HistGeom &g, const HistForm &f, size_t scratch_bytes) {
  if (!store_ok(s) || !f.ok() || g.col0 < 0 || g.span < 1 || (int64_t)g.col0 + g.span > s.n || g.width < 1 ||
      g.width > g.span || g.det < 0 || g.det > 2 || g.m < 1 || g.lines < 1 || g.oldest < 0 || g.seen < g.oldest ||
      g.seen - g.oldest > s.cap)
    return false;
  const HistForm w = choose_history(g.lines, g.m, g.span, g.width, s.q.format);
  if (w.kind != f.kind || w.px != f.px || w.tiles != f.tiles || w.lines != f.lines || w.k != f.k || w.s != f.s ||
      w.slice_rows != f.slice_rows || w.gy != f.gy)
    return false;
  const int bmax = (g.span + g.width - 1) / g.width;
  const int room = hist_tile_cols(s.q.format) - (hist_lane_cols(s.q.format) - 1);
  if (!(f.px == 1 || f.px * bmax <= room) || (int64_t)f.px * f.tiles < g.width || f.tiles > 65535 || f.gy < 1)
    return false;
  if (f.kind == kHistWhole ? ((int64_t)f.gy * f.k < g.lines || f.s != 1)
                           : ((int64_t)f.s * f.slice_rows < g.m || f.gy != g.lines * f.s))
    return false;
  return scratch_bytes >= history_scratch_bytes(f, g.width);
}

}  // namespace

// (sized for the widest partial, a float64 sum)
size_t history_scratch_bytes(const HistForm &f, int width) {
  return f.kind == kHistSliced ? (size_t)f.lines * f.s * width * sizeof(double) : 0;
}

hipError_t launch_history_pack(const float *rows, int n_win, int count, int64_t row0, const HistStore &s,
                               hipStream_t st) {
  if (!rows || !store_ok(s) || n_win < s.n || count < 1 || count > s.cap || row0 < 0) return hipErrorInvalidValue;
  const int vec = n_win % 4 == 0 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0;
  const dim3 grid((unsigned)((s.stride / 4 + 255) / 256), (unsigned)std::min(count, 32768)), block(256);
  if (s.q.format == kHistF32)
    hipLaunchKernelGGL(history_pack_kernel<kHistF32>, grid, block, 0, st, rows, n_win, count, row0 % s.cap, s, vec);
  else if (s.q.format == kHistU16)
    hipLaunchKernelGGL(history_pack_kernel<kHistU16>, grid, block, 0, st, rows, n_win, count, row0 % s.cap, s, vec);
  else
    hipLaunchKernelGGL(history_pack_kernel<kHistU8>, grid, block, 0, st, rows, n_win, count, row0 % s.cap, s, vec);
  return hipGetLastError();
}

hipError_t launch_history_unpack(const HistStore &s, int64_t row0, int count, int n_win, float *rows, hipStream_t st) {
  if (!rows || !store_ok(s) || n_win < s.n || count < 1 || count > s.cap || row0 < 0) return hipErrorInvalidValue;
  const int vec = n_win % 4 == 0 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0;
  const dim3 grid((unsigned)(((s.n + 3) / 4 + 255) / 256), (unsigned)std::min(count, 32768)), block(256);
  if (s.q.format == kHistF32)
    hipLaunchKernelGGL(history_unpack_kernel<kHistF32>, grid, block, 0, st, s, row0 % s.cap, count, n_win, rows, vec);
  else if (s.q.format == kHistU16)
    hipLaunchKernelGGL(history_unpack_kernel<kHistU16>, grid, block, 0, st, s, row0 % s.cap, count, n_win, rows, vec);
  else
    hipLaunchKernelGGL(history_unpack_kernel<kHistU8>, grid, block, 0, st, s, row0 % s.cap, count, n_win, rows, vec);
  return hipGetLastError();
}

#define ZFFT_HIST_DISPATCH(KERNEL, ...)                                                      \
  do {                                                                                       \
    const int fd = s.q.format * 3 + g.det;                                                   \
    switch (fd) {                                                                            \
      case 0: hipLaunchKernelGGL((KERNEL<kHistF32, 0>), grid, block, 0, st, __VA_ARGS__); break; \
      case 1: hipLaunchKernelGGL((KERNEL<kHistF32, 1>), grid, block, 0, st, __VA_ARGS__); break; \
      case 2: hipLaunchKernelGGL((KERNEL<kHistF32, 2>), grid, block, 0, st, __VA_ARGS__); break; \
      case 3: hipLaunchKernelGGL((KERNEL<kHistU16, 0>), grid, block, 0, st, __VA_ARGS__); break; \
      case 4: hipLaunchKernelGGL((KERNEL<kHistU16, 1>), grid, block, 0, st, __VA_ARGS__); break; \
      case 5: hipLaunchKernelGGL((KERNEL<kHistU16, 2>), grid, block, 0, st, __VA_ARGS__); break; \
      case 6: hipLaunchKernelGGL((KERNEL<kHistU8, 0>), grid, block, 0, st, __VA_ARGS__); break;  \
      case 7: hipLaunchKernelGGL((KERNEL<kHistU8, 1>), grid, block, 0, st, __VA_ARGS__); break;  \
      default: hipLaunchKernelGGL((KERNEL<kHistU8, 2>), grid, block, 0, st, __VA_ARGS__); break; \
    }                                                                                        \
  } while (0)

hipError_t launch_history_view(const HistStore &s, const HistGeom &g, const HistForm &f, float *img, void *scratch,
                               size_t scratch_bytes, hipStream_t st) {
  if (!img || !view_ok(s, g, f, scratch_bytes) || (f.kind == kHistSliced && !scratch)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)f.gy, (unsigned)f.tiles), block(64 * kHistWaves);
  ZFFT_HIST_DISPATCH(history_view_kernel, s, g, f, img, scratch);
  return hipGetLastError();
}

hipError_t launch_history_finish(const HistStore &s, const HistGeom &g, const HistForm &f, float *img,
                                 const void *scratch, size_t scratch_bytes, hipStream_t st) {
  if (!img || !scratch || !view_ok(s, g, f, scratch_bytes) || f.kind != kHistSliced) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(((int64_t)g.lines * g.width + 255) / 256)), block(256);
  ZFFT_HIST_DISPATCH(history_finish_kernel, s, g, f, img, scratch);
  return hipGetLastError();
}

#undef ZFFT_HIST_DISPATCH

}  // namespace zfft
