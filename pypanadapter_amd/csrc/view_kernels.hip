// view_kernels.hip -- the display viewport of libzfft.so: pushed rows reduced to a pixel grid on
// the device (rule: zfft.h, zfft_plan_viewport; entry points: zfft_viewport.cpp; chooser:
// zfft_view_plan.h).  A file of its own, so the code objects of the other kernel
// files stay as they were.
//
// view_lines_kernel.  A workgroup of four waves owns one column tile -- px consecutive pixels,
// at most 256 row columns, starting and ending on bucket edges -- and a run of groups (or, in
// the split form, one slice of one group's rows).  Lane l of a wave reads columns c0 + l,
// c0 + 64 + l, ... of a row: 256-byte coalesced loads, U = 4 rows in flight per wave and load
// slot.  The rows of a group are reduced elementwise in registers (four accumulators per lane,
// one per 64-column chunk; a bucket wider than 256 columns folds onto them, px = 1), the waves
// of a team are combined in LDS into one column-resolution reduced row, and pixel thread t then
// reduces its bucket from LDS.  Short groups (one wave per group, a kernel of its own) skip the
// workgroup: a wave reduces its group's rows, passes them through its own LDS row and reduces
// the buckets itself, lane l the pixels l + 64 i, with no workgroup barrier inside the loop; its
// hold partials meet the other waves' through LDS once at the end.  A line complete within the push goes to its ring slot at once
// (the slots of a push's lines are distinct: only the last H are written), the newest to `last`,
// and the workgroup keeps the fmax / fmin of its lines for the hold traces.  What is not a whole
// line -- the group the pending rows began, the group the push leaves incomplete, every slice of
// the split form -- goes to the plan's scratch as a raw partial: the value for MAX / MIN, the
// float64 linear sum for MEAN.
// view_finish_kernel.  Per pixel: merges the pending accumulator into the first group, combines
// the split form's slices, writes those lines in order, stores the new pending group and folds
// the workgroups' hold partials into max_hold / min_hold.
// No workgroup waits for another and there is no atomic: fmax and fmin do not depend on the
// order, so MAX and MIN are the same bits however a push is split.
//
// MEAN: 10^(v/20) as exp2f(v * log2(10)/20) in float32 (argument rounding 1.3e-6 relative at
// -160 dB), four rows summed in float32, every further sum in float64; 20 log10(sum / |S|) in
// float64, rounded once.  NaN, +inf and the 0 of -inf travel through the sums unaided.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "zfft_internal.h"

namespace zfft {

namespace {

constexpr int kU = 4;  // rows a wave loads at once per 64-column chunk
constexpr int kSlots = kViewTileCols, kChunks = kViewTileCols / 64;
static_assert(kChunks == 4 && kViewWaves == 4, "four chunks per lane, four waves per workgroup");

template <int DET>
struct Red {
  using T = float;
  static __device__ __forceinline__ T ident() { return __builtin_nanf(""); }
  static __device__ __forceinline__ T comb(T a, T b) { return DET == 0 ? fmaxf(a, b) : fminf(a, b); }
  static __device__ __forceinline__ float fin(T a, double) { return a; }
};
template <>
struct Red<2> {
  using T = double;
  static __device__ __forceinline__ T ident() { return 0.0; }
  static __device__ __forceinline__ T comb(T a, T b) { return a + b; }
  static __device__ __forceinline__ float fin(T a, double n) { return (float)(20.0 * log10(a / n)); }
};

__device__ __forceinline__ int vedge(const ViewGeom &g, int x) {
  return g.col0 + (int)((int64_t)x * g.span / g.width);
}
// Ring slot of the push's line r: the slot that is image row H - 1 (scroll +1) or 0 (scroll -1)
// once off has advanced by its r + 1 lines, img[i] == ring[(i + off) mod H].  For scroll -1 that
// is waterfall_rows_kernel's slot; for +1 it is one further (the reference's roll leaves its
// newest line at row H - 2 and the oldest at H - 1, a quirk a display has no use for).
__device__ __forceinline__ int vslot(const ViewGeom &g, int r) {
  int s = (int)((g.H - 1 + (int64_t)g.off0 + (int64_t)r * g.scroll + (g.scroll > 0 ? 1 : 0)) % g.H);
  return s < 0 ? s + g.H : s;
}

// What a pixel thread does with a finished line r of this push.
struct Emit {
  float *ring, *last;
  float hmax, hmin;
  __device__ __forceinline__ void line(const ViewGeom &g, int r, int x, float v, float &hx, float &hn) {
    if (r >= g.ncomp - g.H) ring[(int64_t)vslot(g, r) * g.width + x] = v;
    if (r == g.ncomp - 1) last[x] = v;
    hx = fmaxf(hx, v);
    hn = fminf(hn, v);
  }
  __device__ __forceinline__ void line(const ViewGeom &g, int r, int x, float v) { line(g, r, x, v, hmax, hmin); }
};

// LDS written by a wave is read by other lanes of the same wave: no workgroup barrier needed
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int DET, int TEAM>
__global__ __launch_bounds__(64 * kViewWaves) void view_lines_kernel(const float *__restrict__ rows, ViewGeom g,
                                                                      ViewForm f, float *__restrict__ ring,
                                                                      float *__restrict__ tr, void *__restrict__ scratch) {
  using R = Red<DET>;
  using T = typename R::T;
  __shared__ T lds[kViewWaves][kSlots];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int x0 = blockIdx.y * f.px, x1 = min(g.width, x0 + f.px), npx = x1 - x0;
  const int c0 = vedge(g, x0), ncols = vedge(g, x1) - c0;
  const bool folded = ncols > kSlots;  // (then px = 1: every column is pixel x0's)
  constexpr int team = TEAM, ng = kViewWaves / team;  // (a kernel each: the team of four carries no per-wave pixel state)
  const int gs = wave / team, wt = wave % team;
  const bool split = f.kind == kViewSplit;
  // the groups of this workgroup: [j0, j1), ng at a time (split: the one group of its slice)
  const int j0 = split ? (int)blockIdx.x / f.s : (int)min((int64_t)blockIdx.x * f.k, (int64_t)f.groups);
  const int j1 = split ? j0 + 1 : (int)min((int64_t)j0 + f.k, (int64_t)f.groups);
  const int kk = split ? (int)blockIdx.x % f.s : 0;
  const float *base = rows + c0;
  // my pixel (threads t < npx)
  const int x = x0 + tid;
  int b0 = 0, b1 = 0;
  if (tid < npx) {
    b0 = folded ? 0 : vedge(g, x) - c0;
    b1 = folded ? 1 : vedge(g, x + 1) - c0;
  }
  const double cells = tid < npx ? (double)g.m * (double)(vedge(g, x + 1) - vedge(g, x)) : 1.0;
  Emit em{ring, tr, __builtin_nanf(""), __builtin_nanf("")};
  T *edge = static_cast<T *>(scratch);  // lines: [2][width]; split: [groups * s][width]
  // one wave per group (team 1): the wave reduces its own group's buckets too, lane l the pixels
  // x0 + l + 64 i -- no workgroup barrier inside the loop; its hold partials meet at the end
  int wb0[kChunks], wb1[kChunks], wbk[kChunks];
  float whx[kChunks], whn[kChunks];
#pragma unroll
  for (int i = 0; i < kChunks; ++i) {
    const int p = lane + 64 * i;
    wb0[i] = wb1[i] = 0;
    wbk[i] = 1;
    whx[i] = whn[i] = __builtin_nanf("");
    if (team == 1 && p < npx) {
      const int e0 = vedge(g, x0 + p), e1 = vedge(g, x0 + p + 1);
      wb0[i] = folded ? 0 : e0 - c0;
      wb1[i] = folded ? 1 : e1 - c0;
      wbk[i] = e1 - e0;
    }
  }

  for (int jb = j0; jb < j1; jb += ng) {
    // ---- the rows [ra, rb) of the push that this wave's group (slice) holds
    const int j = jb + gs;
    int ra = 0, rb = 0;
    if (j < j1) {
      int64_t ga = (int64_t)j * g.m, gb = ga + g.m;  // in rows counted from the pending group's first
      if (split) {
        ga += (int64_t)kk * f.slice_rows;
        gb = min(gb, ga + f.slice_rows);
      }
      ra = (int)max((int64_t)0, ga - g.pending);
      rb = (int)min((int64_t)g.count, gb - g.pending);
      if (rb < ra) rb = ra;
    }
    T acc[kChunks];
#pragma unroll
    for (int i = 0; i < kChunks; ++i) acc[i] = R::ident();
    for (int cb = 0; cb < ncols; cb += kSlots) {
      const int nch = min(kChunks, (ncols - cb + 63) >> 6);
      for (int r = ra + wt * kU; r < rb; r += team * kU) {
        // clamped addresses stay inside the group's rows and the tile's columns: a duplicate is
        // harmless to fmax / fmin, MEAN masks it
        float v[kU][kChunks];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const float *pr = base + (int64_t)min(r + u, rb - 1) * g.n_win;
          if (u == 0 || r + u < rb) {  // (uniform: a short group's missing rows are not loaded)
#pragma unroll
            for (int i = 0; i < kChunks; ++i)
              if (i < nch) v[u][i] = pr[min(cb + 64 * i + lane, ncols - 1)];
          } else {
#pragma unroll
            for (int i = 0; i < kChunks; ++i)
              if (i < nch) v[u][i] = v[0][i];
          }
        }
#pragma unroll
        for (int i = 0; i < kChunks; ++i) {
          if (i < nch) {
            if constexpr (DET == 2) {
              const bool colok = cb + 64 * i + lane < ncols;
              float s = 0.f;
#pragma unroll
              for (int u = 0; u < kU; ++u)
                s += (colok && r + u < rb) ? exp2f(v[u][i] * 0.16609640474436813f) : 0.f;
              acc[i] += (double)s;
            } else {
#pragma unroll
              for (int u = 0; u < kU; ++u) acc[i] = R::comb(acc[i], v[u][i]);
            }
          }
        }
      }
    }
    // ---- one column-resolution reduced row per group in lds[gs * team]
#pragma unroll
    for (int i = 0; i < kChunks; ++i) lds[wave][64 * i + lane] = acc[i];
    if (team == 1) {
      wave_sync();
      if (folded) {
        T a = R::comb(R::comb(lds[wave][lane], lds[wave][64 + lane]),
                      R::comb(lds[wave][128 + lane], lds[wave][192 + lane]));
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) a = R::comb(a, __shfl_xor(a, d));
        wave_sync();  // every lane has read before lane 0 writes
        if (lane == 0) lds[wave][0] = a;
        wave_sync();
      }
      if (j < j1) {
#pragma unroll
        for (int i = 0; i < kChunks; ++i) {
          const int xx = x0 + lane + 64 * i;
          if (lane + 64 * i < npx) {
            T a = R::ident();
            for (int c = wb0[i]; c < wb1[i]; ++c) a = R::comb(a, lds[wave][c]);
            if (j < g.ncomp && (j > 0 || g.pending == 0))
              em.line(g, j, xx, R::fin(a, (double)g.m * (double)wbk[i]), whx[i], whn[i]);
            else
              edge[(int64_t)((j == 0 && g.pending > 0) ? 0 : 1) * g.width + xx] = a;
          }
        }
      }
      wave_sync();  // lds[wave] is this wave's next group's
      continue;
    }
    __syncthreads();
    if (team == kViewWaves) {
      const T a = R::comb(R::comb(lds[0][tid], lds[1][tid]), R::comb(lds[2][tid], lds[3][tid]));
      __syncthreads();
      lds[0][tid] = a;
      __syncthreads();
    }
    if (folded) {
      if (wt == 0) {
        T a = R::comb(R::comb(lds[wave][lane], lds[wave][64 + lane]),
                      R::comb(lds[wave][128 + lane], lds[wave][192 + lane]));
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) a = R::comb(a, __shfl_xor(a, d));
        if (lane == 0) lds[wave][0] = a;
      }
      __syncthreads();
    }
    // ---- buckets, then where the value goes
    if (tid < npx) {
      for (int q = 0; q < ng; ++q) {
        const int jq = jb + q;
        if (jq >= j1) break;
        T a = R::ident();
        for (int c = b0; c < b1; ++c) a = R::comb(a, lds[q * team][c]);
        if (split) {
          edge[(int64_t)blockIdx.x * g.width + x] = a;
        } else if (jq < g.ncomp && (jq > 0 || g.pending == 0)) {
          em.line(g, jq, x, R::fin(a, cells));
        } else {
          edge[(int64_t)((jq == 0 && g.pending > 0) ? 0 : 1) * g.width + x] = a;
        }
      }
    }
    __syncthreads();  // lds is the next groups'
  }
  if (team == 1) {
    float *hl = reinterpret_cast<float *>(&lds[0][0]);  // (at least 4 x 256 floats)
    float hh[2] = {em.hmax, em.hmin};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      __syncthreads();  // every wave is done with lds
#pragma unroll
      for (int i = 0; i < kChunks; ++i) hl[wave * kSlots + 64 * i + lane] = k == 0 ? whx[i] : whn[i];
      __syncthreads();
      for (int w = 0; w < kViewWaves; ++w)
        hh[k] = k == 0 ? fmaxf(hh[k], hl[w * kSlots + tid]) : fminf(hh[k], hl[w * kSlots + tid]);
    }
    em.hmax = hh[0];
    em.hmin = hh[1];
  }
  if (!split && tid < npx) {
    if (g.direct) {  // the only workgroup of its tile and no partial group: the traces here
      float *mx = tr + g.width, *mn = tr + 2 * (int64_t)g.width;
      mx[x] = fmaxf(mx[x], em.hmax);
      mn[x] = fminf(mn[x], em.hmin);
    } else {
      float *hold = reinterpret_cast<float *>(static_cast<double *>(scratch) + 2 * (int64_t)g.width);
      hold[(int64_t)blockIdx.x * g.width + x] = em.hmax;
      hold[((int64_t)f.gy + blockIdx.x) * g.width + x] = em.hmin;
    }
  }
}

// 32 pixels x 8 lanes per workgroup: the lanes of a pixel share the walk over the workgroups'
// hold partials (or a split group's slices), which is a chain of dependent loads per thread
// otherwise -- 544 deep for cfg2's lines -- and lane 0 combines them through LDS and does the rest.
constexpr int kFinPx = 32, kFinLanes = 8;

template <int DET>
__global__ __launch_bounds__(kFinPx *kFinLanes) void view_finish_kernel(ViewGeom g, ViewForm f, float *__restrict__ ring,
                                                                        float *__restrict__ tr, void *__restrict__ pend,
                                                                        const void *__restrict__ scratch) {
  using R = Red<DET>;
  using T = typename R::T;
  __shared__ T red[kFinLanes][kFinPx];
  __shared__ float hm[2][kFinLanes][kFinPx];
  const int px = threadIdx.x % kFinPx, yl = threadIdx.x / kFinPx;
  const int x = min(blockIdx.x * kFinPx + px, g.width - 1);  // (threads past the width repeat the last pixel's loads)
  const bool lead = yl == 0 && (int)(blockIdx.x * kFinPx + px) < g.width;
  const double cells = (double)g.m * (double)(vedge(g, x + 1) - vedge(g, x));
  float *mx = tr + g.width, *mn = tr + 2 * (int64_t)g.width;
  const float nan = __builtin_nanf("");
  Emit em{ring, tr, lead ? mx[x] : nan, lead ? mn[x] : nan};
  T *pd = static_cast<T *>(pend);
  const T *part = static_cast<const T *>(scratch);
  if (f.kind == kViewSplit) {
    for (int j = 0; j < f.groups; ++j) {
      T a = R::ident();
      const T *pj = part + (int64_t)j * f.s * g.width + x;
#pragma unroll 8
      for (int k = yl; k < f.s; k += kFinLanes) a = R::comb(a, pj[(int64_t)k * g.width]);
      red[yl][px] = a;
      __syncthreads();
      if (lead) {
        T b = (j == 0 && g.pending > 0) ? pd[x] : R::ident();
#pragma unroll
        for (int l = 0; l < kFinLanes; ++l) b = R::comb(b, red[l][px]);
        if (j < g.ncomp)
          em.line(g, j, x, R::fin(b, cells));
        else
          pd[x] = b;
      }
      __syncthreads();  // red is the next group's
    }
  } else {
    const float *hold = reinterpret_cast<const float *>(static_cast<const double *>(scratch) + 2 * (int64_t)g.width);
    float hmax = nan, hmin = nan;
#pragma unroll 8
    for (int y = yl; y < f.gy; y += kFinLanes) {
      hmax = fmaxf(hmax, hold[(int64_t)y * g.width + x]);
      hmin = fminf(hmin, hold[((int64_t)f.gy + y) * g.width + x]);
    }
    hm[0][yl][px] = hmax;
    hm[1][yl][px] = hmin;
    __syncthreads();
    if (lead) {
      if (g.pending > 0) {  // the group the pending rows began
        const T a = R::comb(pd[x], part[x]);
        if (g.ncomp >= 1)
          em.line(g, 0, x, R::fin(a, cells));
        else
          pd[x] = a;
      }
#pragma unroll
      for (int l = 0; l < kFinLanes; ++l) {
        em.hmax = fmaxf(em.hmax, hm[0][l][px]);
        em.hmin = fminf(em.hmin, hm[1][l][px]);
      }
      // the group the push leaves incomplete (when it is not the pending one again)
      if (((int64_t)g.pending + g.count) % g.m != 0 && !(g.ncomp == 0 && g.pending > 0)) pd[x] = part[g.width + x];
    }
  }
  if (lead) {
    mx[x] = em.hmax;
    mn[x] = em.hmin;
  }
}

__global__ __launch_bounds__(256) void view_fill_kernel(float *__restrict__ p, int64_t n, float v) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = v;
}

}  // namespace

bool view_direct(const ViewGeom &g, const ViewForm &f) {
  return f.kind == kViewLines && f.gy == 1 && g.pending == 0 && g.count % g.m == 0;
}

size_t view_scratch_bytes(const ViewForm &f, int width) {
  if (f.kind == kViewSplit) return (size_t)f.groups * f.s * width * sizeof(double);
  return (size_t)2 * width * sizeof(double) + (size_t)2 * f.gy * width * sizeof(float);
}

// The form must be choose_view's for this push (recomputed here: the grid and the scratch layout
// follow from it), the window inside a row, the scratch large enough.
static bool view_args_ok(const ViewGeom &g, const ViewForm &f, size_t scratch_bytes) {
  if (!f.ok() || g.count < 1 || g.m < 1 || g.pending < 0 || g.pending >= g.m || g.col0 < 0 || g.span < 1 ||
      g.width < 1 || g.width > g.span || (int64_t)g.col0 + g.span > g.n_win || g.H < 1 || g.det < 0 || g.det > 2 ||
      (g.scroll != 1 && g.scroll != -1) || g.off0 < 0 || g.off0 >= g.H)
    return false;
  const ViewForm w = choose_view(g.count, g.m, g.pending, g.span, g.width);
  if (w.kind != f.kind || w.team != f.team || w.px != f.px || w.tiles != f.tiles || w.groups != f.groups ||
      w.k != f.k || w.s != f.s || w.slice_rows != f.slice_rows || w.gy != f.gy)
    return false;
  const int bmax = (g.span + g.width - 1) / g.width;
  if (!(f.px == 1 || f.px * bmax <= kViewTileCols) || (int64_t)f.px * f.tiles < g.width || f.tiles > 65535 || f.gy < 1)
    return false;
  if (f.kind == kViewLines ? ((int64_t)f.gy * f.k < f.groups || f.s != 1)
                           : ((int64_t)f.s * f.slice_rows < g.m || f.gy != f.groups * f.s || f.team != kViewWaves))
    return false;
  if (g.ncomp != (int)(((int64_t)g.pending + g.count) / g.m) || g.direct != (view_direct(g, f) ? 1 : 0)) return false;
  return scratch_bytes >= view_scratch_bytes(f, g.width);
}

hipError_t launch_view_lines(const float *rows, const ViewGeom &g, const ViewForm &f, float *ring, float *traces,
                             void *scratch, size_t scratch_bytes, hipStream_t st) {
  if (!rows || !ring || !traces || !scratch || !view_args_ok(g, f, scratch_bytes)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)f.gy, (unsigned)f.tiles), block(64 * kViewWaves);
#define ZFFT_VIEW_LINES(DET, TEAM)       \
  if (g.det == DET && f.team == TEAM)   \
    hipLaunchKernelGGL((view_lines_kernel<DET, TEAM>), grid, block, 0, st, rows, g, f, ring, traces, scratch);
  ZFFT_VIEW_LINES(0, 1)
  ZFFT_VIEW_LINES(0, 4)
  ZFFT_VIEW_LINES(1, 1)
  ZFFT_VIEW_LINES(1, 4)
  ZFFT_VIEW_LINES(2, 1)
  ZFFT_VIEW_LINES(2, 4)
#undef ZFFT_VIEW_LINES
  return hipGetLastError();
}

hipError_t launch_view_finish(const ViewGeom &g, const ViewForm &f, float *ring, float *traces, void *pend,
                              const void *scratch, size_t scratch_bytes, hipStream_t st) {
  if (!ring || !traces || !pend || !scratch || !view_args_ok(g, f, scratch_bytes) || g.direct) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((g.width + kFinPx - 1) / kFinPx)), block(kFinPx * kFinLanes);
  if (g.det == 0)
    hipLaunchKernelGGL(view_finish_kernel<0>, grid, block, 0, st, g, f, ring, traces, pend, scratch);
  else if (g.det == 1)
    hipLaunchKernelGGL(view_finish_kernel<1>, grid, block, 0, st, g, f, ring, traces, pend, scratch);
  else
    hipLaunchKernelGGL(view_finish_kernel<2>, grid, block, 0, st, g, f, ring, traces, pend, scratch);
  return hipGetLastError();
}

hipError_t launch_view_fill(float *p, int64_t n, float v, hipStream_t st) {
  if (!p || n < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(view_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p, n, v);
  return hipGetLastError();
}

}  // namespace zfft
