// detect_local_kernels.hip -- the row detector's local noise floor (order-statistic CFAR): per
// column the value of rank floor(q (m - 1)) among the m finite values of its reference cells,
// the half_window columns beyond `guard` columns on either side, cut at the row's ends (rule:
// zfft.h, zfft_plan_detect_local; entry points: zfft_detect.cpp; chooser: zfft_detect_plan.h;
// DESIGN §3.3.7).  A file of its own, so the code objects of the other kernel files stay as
// they were.  The on-flags, runs, records and occupancy are detect_kernels.hip's, given these
// floors (its LOCAL instantiations).
//
// The grid runs over (row, tile of 256 columns), so one wide row -- the UI's case -- spreads over
// as many CUs as it has tiles instead of one workgroup.  A workgroup loads its tile and a halo of
// guard + half_window columns on either side once, as detect_kernels.hip's order-preserving keys
// (the columns outside the row as the pad key, which is not finite), and keeps them in LDS
// bit-sliced: plane b holds bit b of every cell's key, one bit per cell, and plane 32 whether the
// cell is finite -- 33 ballots per 64 cells, 3.4 KB in all.
//
// A thread owns a column.  Its window in a plane is two runs of half_window bits, each cut out
// of the plane's words by funnel shifts (all 32 lanes of a half-wave read the same words: a
// broadcast, no bank conflict).  The selection is a radix select on bit masks: the candidates
// start as the window's finite cells (their number is m), and for each key bit from the top the
// candidates with a 0 there are `cand & ~plane`, counted by a population count; if the rank lies
// beyond them the floor's bit is 1 and the candidates are narrowed to the others, else to them.
// A step is a handful of word operations whatever half_window is up to 32 (SW = 1 word per
// side), twice that up to 64, four times up to 128 -- not 2 half_window compares: the first
// form of this kernel swept the keys (34 sweeps of 2 half_window compares per column) and ran
// at the LDS read rate or, with the window in registers, at the compare's carry hazard (DESIGN
// §3.3.7).  Ties need no care, a flat floor costs what noise costs, and there is no barrier and
// no atomic in the selection.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "zfft.h"
#include "zfft_detect_keys.h"
#include "zfft_internal.h"

namespace zfft {

namespace {

using u64 = unsigned long long;

constexpr int kPlanes = 33;  // the key's 32 bits, then "finite"
// 32-bit words of a plane: 768 cells (the tile and two halos of 256 at most), then two words
// that stay zero, so that a window's last funnel shift reads inside the plane
constexpr int kPlaneWords = 26;
constexpr int kMaxCells = kDetectLocalTile + 2 * (kDetectLocalMaxHalf + kDetectLocalMaxGuard);
static_assert(kMaxCells == 32 * (kPlaneWords - 2) && kMaxCells % 64 == 0, "a plane holds every cell");
static_assert(kPlaneWords % 2 == 0, "a ballot is stored as one aligned 64-bit word");

template <int SW>
__global__ __launch_bounds__(kDetectLocalTile) void detect_floor_kernel(const float *__restrict__ rows,
                                                                        int64_t row_stride, int64_t ntiles, int tiles,
                                                                        int row_len, int h, int gd, double q,
                                                                        float *__restrict__ floors,
                                                                        int64_t floor_stride) {
  constexpr int TILE = kDetectLocalTile;
  __shared__ __attribute__((aligned(8))) uint32_t s_pl[kPlanes][kPlaneWords];  // cell i is column tile0 - halo + i
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int halo = h + gd, ncells = TILE + 2 * halo;  // <= kMaxCells
  if (threadIdx.x < kPlanes) s_pl[threadIdx.x][kPlaneWords - 2] = s_pl[threadIdx.x][kPlaneWords - 1] = 0;
  // This thread's window: the h cells from a0 (columns j - gd - h .. j - gd - 1) and the h from
  // a1 (j + gd + 1 .. j + gd + h); a1 + h <= ncells.  Word k of a side is bits [32 k, 32 k + 32)
  // of the run, those at or beyond h masked off.
  const int a0 = threadIdx.x, a1 = halo + threadIdx.x + gd + 1;
  const int w0 = a0 >> 5, sh0 = a0 & 31, w1 = a1 >> 5, sh1 = a1 & 31;  // w1 + SW + 1 <= kPlaneWords
  uint32_t msk[SW];
#pragma unroll
  for (int k = 0; k < SW; ++k) {
    const int r = h - 32 * k;
    msk[k] = r >= 32 ? ~0u : r <= 0 ? 0u : (1u << r) - 1u;
  }
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {  // the same trips for every thread
    const int64_t row = t / tiles;
    const int tile0 = (int)(t - row * tiles) * TILE;
    const float *p = rows + row * row_stride;
    // ---- the planes: wave w takes the 64-cell chunks w, w + 4, ... that hold a cell (the words
    // beyond stay as they are: no window reaches them unmasked)
    for (int chunk = wave; chunk * 64 < ncells; chunk += TILE / 64) {
      const int i = chunk * 64 + lane, c = tile0 - halo + i;
      const uint32_t key = (i < ncells && c >= 0 && c < row_len) ? det_key(p[c]) : kKeyPad;
      u64 mine = __ballot(key >= kKeyFiniteLo && key < kKeyFiniteHi);  // lane 32's: the finite plane
#pragma unroll 8  // (32 ballots in flight spill their scalar pairs)
      for (int b = 0; b < 32; ++b) {
        const u64 bal = __ballot((key >> b) & 1u);
        if (lane == b) mine = bal;
      }
      if (lane < kPlanes) *reinterpret_cast<u64 *>(&s_pl[lane][2 * chunk]) = mine;  // 2 chunk + 1 < kPlaneWords - 2
    }
    __syncthreads();
    const int j = tile0 + (int)threadIdx.x;
    if (j < row_len) {
      auto left = [&](int pl, int k) -> uint32_t {
        return __builtin_amdgcn_alignbit(s_pl[pl][w0 + k + 1], s_pl[pl][w0 + k], sh0);
      };
      auto right = [&](int pl, int k) -> uint32_t {
        return __builtin_amdgcn_alignbit(s_pl[pl][w1 + k + 1], s_pl[pl][w1 + k], sh1);
      };
      uint32_t cl[SW], cr[SW];  // the candidates: at first the window's finite cells
      int m = 0;
#pragma unroll
      for (int k = 0; k < SW; ++k) {
        cl[k] = left(32, k) & msk[k];
        cr[k] = right(32, k) & msk[k];
        m += __popc(cl[k]) + __popc(cr[k]);
      }
      float floorv = __uint_as_float(0x7FC00000u);  // m == 0: NaN
      if (m > 0) {  // (per thread: no barrier below)
        const int kth = (int)(long long)floor(q * (double)(m - 1));
        uint32_t ans = 0;
        int less = 0;  // candidates dropped so far as smaller than the floor
        for (int b = 31; b >= 0; --b) {
          uint32_t zl[SW], zr[SW];  // the candidates with bit b clear: the smaller ones
          int cnt = 0;
#pragma unroll
          for (int k = 0; k < SW; ++k) {
            zl[k] = cl[k] & ~left(b, k);
            zr[k] = cr[k] & ~right(b, k);
            cnt += __popc(zl[k]) + __popc(zr[k]);
          }
          const bool one = less + cnt <= kth;  // the rank lies beyond them: the floor's bit is 1
          if (one) {
            ans |= 1u << b;
            less += cnt;
          }
#pragma unroll
          for (int k = 0; k < SW; ++k) {
            cl[k] = one ? cl[k] ^ zl[k] : zl[k];
            cr[k] = one ? cr[k] ^ zr[k] : zr[k];
          }
        }
        floorv = det_value(ans);
      }
      floors[row * floor_stride + j] = floorv;
    }
    __syncthreads();  // the planes are the next tile's
  }
}

template <int SW>
hipError_t launch_words(const float *rows, int64_t row_stride, int64_t ntiles, int row_len, int h, int gd, double q,
                        const DetectLocalForm &f, float *floors, int64_t floor_stride, hipStream_t st) {
  hipLaunchKernelGGL((detect_floor_kernel<SW>), dim3((unsigned)f.grid), dim3(kDetectLocalTile), 0, st, rows, row_stride,
                     ntiles, f.tiles, row_len, h, gd, q, floors, floor_stride);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_detect_floors(const float *rows, int64_t row_stride, int count, int row_len, int half_window,
                                int guard, double q, const DetectLocalForm &f, float *floors, int64_t floor_stride,
                                hipStream_t st) {
  const int64_t ntiles = (int64_t)count * f.tiles;
  if (!f.ok() || !rows || !floors || count < 1 || count > f.chunk_rows || row_len < 1 || row_len > kDetectMaxCols ||
      row_stride < row_len || floor_stride < row_len || half_window < 1 || half_window > kDetectLocalMaxHalf ||
      guard < 0 || guard > kDetectLocalMaxGuard || !(q >= 0.0 && q <= 1.0) || f.tile != kDetectLocalTile ||
      f.halo != guard + half_window || f.lds_keys() > kMaxCells || (int64_t)f.tiles * f.tile < row_len ||
      (int64_t)(f.tiles - 1) * f.tile >= row_len || f.grid < 1 || f.grid > ntiles || f.grid > kDetectLocalGridMax ||
      (f.words != 1 && f.words != 2 && f.words != 4) || half_window > 32 * f.words)
    return hipErrorInvalidValue;
  if (f.words == 1)
    return launch_words<1>(rows, row_stride, ntiles, row_len, half_window, guard, q, f, floors, floor_stride, st);
  if (f.words == 2)
    return launch_words<2>(rows, row_stride, ntiles, row_len, half_window, guard, q, f, floors, floor_stride, st);
  return launch_words<4>(rows, row_stride, ntiles, row_len, half_window, guard, q, f, floors, floor_stride, st);
}

}  // namespace zfft
