// detect_kernels.hip -- the row detector of libzfft.so: per row a noise floor (an exact order
// statistic), the emissions above floor + threshold as records in column order, and a per-column
// occupancy count (rule: zfft.h; entry points: zfft_detect.cpp; chooser: zfft_detect_plan.h;
// DESIGN §3.3.4).  A file of its own, so the code objects of the other kernel files stay as
// they were.
//
// One workgroup of NW waves takes a row at a time and holds it in registers as order-preserving
// keys, PER per lane (zfft_detect_plan.h's layout: word wd = i * NW + wave, lane l its column
// 64 wd + l); the widest form (65,536 columns: 64 keys per lane of 1024 threads) keeps half of
// them in LDS, 128 KB that each thread reads back at its own lane-consecutive addresses.  The
// key map is a bijection of the float's bits, so the values -- NaN payloads and the sign of a
// zero included -- come back out of the keys and the row is read once.
//
// Floor: rank select by bits.  count(key < t) is one compare, one ballot and one population
// count per word, whatever the values are: a flat floor, where most of a row shares its sign,
// exponent and top mantissa bits, costs what uniform noise costs, there is no counter for the
// row to pile onto and no atomic.  32 steps find the largest t with count(key < t) <= rank, which
// is the key of that rank; ties need no care.  With one wave per row (NW = 1) the counts are
// wave-uniform scalars: no LDS, no barrier.  With more waves a step adds the waves' counts
// through LDS, two buffers in turn, one barrier per step.
//
// Runs: a word of on-flags is one ballot, kept in LDS (s_on).  A run start is a set bit whose
// lower neighbour (the previous word's top bit for bit 0) is clear; its lane finds the run's
// last column by scanning words.  Runs shorter than min_width are cleared from a copy (s_keep),
// which then holds exactly the kept runs: its set bits are the occupancy (counted per thread
// over the workgroup's rows, then one vector atomicAdd per non-zero column), its starts the
// emissions.  A start's rank is the exclusive prefix of the words' start counts plus the starts
// below it in its word, so the record slots follow column order whatever the scheduling; no
// atomic append.  The first K runs go to s_run by rank, and each is then
// swept by a whole wave for its peak (first maximum), written as one 16-byte store.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "zfft.h"
#include "zfft_detect_keys.h"  // det_key, det_value, the key ranges
#include "zfft_internal.h"

namespace zfft {

namespace {

using u64 = unsigned long long;

// The last column of the run of set bits that holds bit `lane` of word wd (m: `words` words).
__device__ __forceinline__ int run_last(const u64 *m, int words, int wd, int lane) {
  const u64 inv = ~(m[wd] >> lane);  // bit n: column lane + n is clear (or past the word's end)
  const int n = inv ? __ffsll((long long)inv) - 1 : 64;
  if (lane + n < 64) return wd * 64 + lane + n - 1;
  int w = wd + 1;
  while (w < words && m[w] == ~0ull) ++w;
  if (w == words) return words * 64 - 1;
  return w * 64 + __ffsll((long long)~m[w]) - 2;
}

// The floor's selection: 0 = by bits with ballots (shipped), 1 = 8-bit digit histograms with
// per-wave LDS counters, built for the A/B of DESIGN §3.3.4 (the forms with keys in registers).
#ifndef ZFFT_DETECT_SELECT
#define ZFFT_DETECT_SELECT 0
#endif
constexpr int kDetectSelect = ZFFT_DETECT_SELECT;

// starts of the runs of word `on`; below: the top bit of the word before (0 for the first)
__device__ __forceinline__ u64 run_starts(u64 on, u64 below) { return on & ~((on << 1) | below); }

// LOCAL (zfft_plan_detect_local): column j is on against its own floor, col_floor[row *
// g.n_win + j] (detect_local_kernels.hip wrote it), instead of the row's; everything else,
// the row's floor in floor_out included, is the same code.
template <int NW, int PER, int PL, bool LOCAL>
__global__ __launch_bounds__(64 * NW) void detect_rows_kernel(const float *__restrict__ rows, int64_t row_stride,
                                                              int count, DetectGeom g, float *__restrict__ floor_out,
                                                              int32_t *__restrict__ found_out,
                                                              zfft_emission *__restrict__ events,
                                                              unsigned *__restrict__ occ,
                                                              const float *__restrict__ col_floor) {
  constexpr int WORDS = NW * PER, PR = PER - PL;  // per lane PR keys in registers, PL in LDS
  extern __shared__ uint32_t s_key[];  // [PL][64 NW]: a thread reads back only what it wrote
  __shared__ u64 s_on[WORDS], s_keep[WORDS];
  __shared__ int s_cnt[WORDS];  // kept run starts per word, then their exclusive prefix
  __shared__ int s_part[2][NW];
  __shared__ int s_hist[kDetectSelect == 1 && PL == 0 ? NW : 1][256];  // ZFFT_DETECT_SELECT=1 only
  __shared__ int2 s_run[kDetectMaxPerRow];
  __shared__ int s_found;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int K = g.max_per_row;
  // Occupancy: the counts of this thread's columns over all the workgroup's rows, added to the
  // table once at the end.  One atomicAdd per on column and row put every row of a call onto
  // the table's few cache lines (16 for 512 columns) and took 1.07-1.47 ms for cfg2's rows,
  // whatever the selection.  The widest form has no registers to spare and
  // 2048 lines to spread over: it adds per row.
  constexpr bool ACC = PL == 0;
  unsigned acc[ACC ? PER : 1] = {};

  for (int row = blockIdx.x; row < count; row += gridDim.x) {  // the same trips for every thread
    const float *p = rows + (int64_t)row * row_stride;
    auto load_key = [&](int i) -> uint32_t {
      const int j = (i * NW + wave) * 64 + lane;  // past the row: its last column, loaded and dropped
      const uint32_t k = det_key(p[min(j, g.row_len - 1)]);
      return j < g.row_len ? k : kKeyPad;
    };
    uint32_t key[PR];
#pragma unroll
    for (int i = 0; i < PR; ++i) key[i] = load_key(i);
#pragma unroll 8
    for (int i = 0; i < PL; ++i) s_key[i * (64 * NW) + threadIdx.x] = load_key(PR + i);

    // ---- floor: the key of rank nlow + k, k = floor(q (m - 1)) among the m finite keys
    int step = 0;
    auto count_lt = [&](uint32_t t) -> int {
      int c = 0;
#pragma unroll
      for (int i = 0; i < PR; ++i) c += __popcll(__ballot(key[i] < t));
#pragma unroll 8
      for (int i = 0; i < PL; ++i) c += __popcll(__ballot(s_key[i * (64 * NW) + threadIdx.x] < t));
      if constexpr (NW > 1) {
        int *part = s_part[step++ & 1];
        if (lane == 0) part[wave] = c;
        __syncthreads();
        c = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) c += part[w];
      }
      return c;
    };
    const int nlow = count_lt(kKeyFiniteLo);
    const int m = count_lt(kKeyFiniteHi) - nlow;
    float floorv = __uint_as_float(0x7FC00000u), thr = floorv;  // m == 0: NaN, nothing is on
    if (m > 0) {
      const int rank = nlow + (int)(long long)floor(g.q * (double)(m - 1));
      uint32_t ans = 0;
      if constexpr (kDetectSelect == 1 && PL == 0) {
        // the rejected form: four passes of 8-bit digits, most significant first,
        // each wave counting into 256 LDS counters of its own
        int left = rank;
        uint32_t mask = 0;
        for (int shift = 24; shift >= 0; shift -= 8) {
          for (int c = 0; c < 4; ++c) s_hist[wave][4 * lane + c] = 0;
          __syncthreads();
#pragma unroll
          for (int i = 0; i < PR; ++i)
            if ((key[i] & mask) == ans) atomicAdd(&s_hist[wave][(key[i] >> shift) & 255u], 1);
          __syncthreads();
          int cnt[4], own = 0;  // lane l: the digits 4 l .. 4 l + 3, summed over the waves
          for (int c = 0; c < 4; ++c) {
            cnt[c] = 0;
            for (int w = 0; w < NW; ++w) cnt[c] += s_hist[w][4 * lane + c];
            own += cnt[c];
          }
          int inc = own;
          for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(inc, d);
            if (lane >= d) inc += o;
          }
          int base = inc - own, digit = -1, rest = 0;
          for (int c = 0; c < 4; ++c) {
            if (digit < 0 && left >= base && left < base + cnt[c]) {
              digit = 4 * lane + c;
              rest = left - base;
            }
            base += cnt[c];
          }
          const int src = __ffsll((long long)__ballot(digit >= 0)) - 1;  // the lowest lane that holds the rank
          ans |= (uint32_t)__shfl(digit, src) << shift;
          left = __shfl(rest, src);
          mask |= 255u << shift;
          __syncthreads();
        }
      } else {
        for (int b = 31; b >= 0; --b) {
          const uint32_t t = ans | (1u << b);
          if (count_lt(t) <= rank) ans = t;
        }
      }
      floorv = det_value(ans);
      thr = __fadd_rn(floorv, g.thr_add);
    }
    if (threadIdx.x == 0) floor_out[row] = floorv;

    // ---- on-flags
    auto col_thr = [&](int i) -> float {
      if constexpr (LOCAL) {  // past the row: the last column's floor, against a pad key (never on)
        const int j = min((i * NW + wave) * 64 + lane, g.row_len - 1);
        return __fadd_rn(col_floor[(int64_t)row * g.n_win + j], g.thr_add);  // a NaN floor: never on
      } else {
        return thr;
      }
    };
#pragma unroll
    for (int i = 0; i < PR; ++i) {
      const u64 on = __ballot(det_value(key[i]) >= col_thr(i));
      if (lane == 0) s_on[i * NW + wave] = s_keep[i * NW + wave] = on;
    }
#pragma unroll 8
    for (int i = 0; i < PL; ++i) {
      const u64 on = __ballot(det_value(s_key[i * (64 * NW) + threadIdx.x]) >= col_thr(PR + i));
      if (lane == 0) s_on[(PR + i) * NW + wave] = s_keep[(PR + i) * NW + wave] = on;
    }
    __syncthreads();

    // ---- runs shorter than min_width leave s_keep
    if (g.min_width > 1) {
#pragma unroll 1
      for (int i = 0; i < PER; ++i) {
        const int wd = i * NW + wave;
        const u64 on = s_on[wd];
        if ((run_starts(on, wd ? s_on[wd - 1] >> 63 : 0) >> lane) & 1) {
          const int first = wd * 64 + lane, last = run_last(s_on, WORDS, wd, lane);
          if (last - first + 1 < g.min_width)
            for (int w = wd; w <= last >> 6; ++w) {
              const int lo = w == wd ? lane : 0, hi = w == last >> 6 ? last & 63 : 63;
              const u64 span = (hi == 63 ? ~0ull : (1ull << (hi + 1)) - 1) & ~((1ull << lo) - 1);
              atomicAnd(&s_keep[w], ~span);
            }
        }
      }
      __syncthreads();
    }

    // ---- occupancy, and the kept starts per word
    if constexpr (ACC) {
#pragma unroll
      for (int i = 0; i < PER; ++i) {
        const int wd = i * NW + wave;
        const u64 on = s_keep[wd];
        if (lane == 0) s_cnt[wd] = __popcll(run_starts(on, wd ? s_keep[wd - 1] >> 63 : 0));
        acc[i] += (unsigned)((on >> lane) & 1);
      }
    } else {
#pragma unroll 1
      for (int i = 0; i < PER; ++i) {
        const int wd = i * NW + wave;
        const u64 on = s_keep[wd];
        if (lane == 0) s_cnt[wd] = __popcll(run_starts(on, wd ? s_keep[wd - 1] >> 63 : 0));
        if ((on >> lane) & 1) atomicAdd(occ + wd * 64 + lane, 1u);  // on: a column < row_len <= n_win
      }
    }
    __syncthreads();
    if (wave == 0) {  // exclusive prefix of s_cnt, lane l its CH consecutive words
      constexpr int CH = (WORDS + 63) / 64;
      int own = 0;
      for (int c = 0; c < CH; ++c)
        if (lane * CH + c < WORDS) own += s_cnt[lane * CH + c];
      int inc = own;
      for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
      }
      int run = inc - own;
      for (int c = 0; c < CH; ++c)
        if (lane * CH + c < WORDS) {
          const int t = s_cnt[lane * CH + c];
          s_cnt[lane * CH + c] = run;
          run += t;
        }
      if (lane == 63) s_found = inc;
    }
    __syncthreads();

    // ---- the first K runs, by rank
#pragma unroll 1
    for (int i = 0; i < PER; ++i) {
      const int wd = i * NW + wave;
      const u64 st = run_starts(s_keep[wd], wd ? s_keep[wd - 1] >> 63 : 0);
      if ((st >> lane) & 1) {
        const int rank = s_cnt[wd] + __popcll(st & ((1ull << lane) - 1));
        if (rank < K) s_run[rank] = make_int2(wd * 64 + lane, run_last(s_keep, WORDS, wd, lane));
      }
    }
    __syncthreads();
    const int found = s_found;
    if (threadIdx.x == 0) found_out[row] = found;

    // ---- records: a wave sweeps a run for its first maximum; the slots beyond `found` are zeros
    for (int r = wave; r < K; r += NW) {
      int4 rec = make_int4(0, 0, 0, 0);
      if (r < found) {
        const int2 fl = s_run[r];
        int bcol = INT_MAX;
        float bv = 0.f;
        for (int j = fl.x + lane; j <= fl.y; j += 64) {
          const float v = p[j];
          if (bcol == INT_MAX || v > bv) {
            bv = v;
            bcol = j;
          }
        }
        for (int d = 32; d >= 1; d >>= 1) {
          const float ov = __shfl_xor(bv, d);
          const int oc = __shfl_xor(bcol, d);
          if (oc != INT_MAX && (bcol == INT_MAX || ov > bv || (ov == bv && oc < bcol))) {
            bv = ov;
            bcol = oc;
          }
        }
        rec = make_int4(fl.x, fl.y, bcol, __float_as_int(bv));
      }
      if (lane == 0) *reinterpret_cast<int4 *>(events + (int64_t)row * K + r) = rec;
    }
    __syncthreads();  // s_run, s_found and the masks are the next row's
  }
  if constexpr (ACC) {
#pragma unroll
    for (int i = 0; i < PER; ++i)
      if (acc[i]) atomicAdd(occ + (i * NW + wave) * 64 + lane, acc[i]);  // non-zero: a column < row_len <= n_win
  }
}

template <int NW, int PER, int PL, bool LOCAL>
hipError_t launch_form(const float *rows, int64_t row_stride, int count, const DetectGeom &g, int grid, float *floor_out,
                       int32_t *found_out, zfft_emission *events, unsigned *occ, const float *col_floor,
                       hipStream_t st) {
  constexpr int lds = PL * 64 * NW * (int)sizeof(uint32_t);  // beside 21 KB of static LDS at most
  static bool attr_set = false;
  if (lds > 48 * 1024 && !attr_set) {
    hipError_t e = hipFuncSetAttribute((const void *)detect_rows_kernel<NW, PER, PL, LOCAL>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  hipLaunchKernelGGL((detect_rows_kernel<NW, PER, PL, LOCAL>), dim3((unsigned)grid), dim3(64 * NW), lds, st, rows,
                     row_stride, count, g, floor_out, found_out, events, occ, col_floor);
  return hipGetLastError();
}

}  // namespace

static_assert(sizeof(zfft_emission) == 16, "a record is one 16-byte store");

hipError_t launch_detect_rows(const float *rows, int64_t row_stride, int count, const DetectGeom &g,
                              const DetectForm &f, float *floor_out, int32_t *found_out, zfft_emission *events,
                              unsigned *occ, hipStream_t st, const float *col_floor) {
  if (!f.ok() || count < 1 || f.grid < 1 || f.grid > count || g.row_len < 1 || g.row_len > f.cols() ||
      g.row_len > g.n_win || row_stride < g.row_len || g.max_per_row < 1 || g.max_per_row > kDetectMaxPerRow ||
      g.min_width < 1 || !(g.q >= 0.0 && g.q <= 1.0) || ((uintptr_t)events & 15))
    return hipErrorInvalidValue;
  // (col_floor holds count rows of stride g.n_win, and row_len <= n_win: every read is inside)
#define ZFFT_DETECT_FORM(NW, PER, PL)                                                                        \
  if (f.waves == NW && f.per == PER)                                                                         \
    return col_floor ? launch_form<NW, PER, PL, true>(rows, row_stride, count, g, f.grid, floor_out, found_out, \
                                                      events, occ, col_floor, st)                             \
                     : launch_form<NW, PER, PL, false>(rows, row_stride, count, g, f.grid, floor_out,        \
                                                       found_out, events, occ, nullptr, st);
  ZFFT_DETECT_FORM(1, 1, 0)
  ZFFT_DETECT_FORM(1, 2, 0)
  ZFFT_DETECT_FORM(1, 4, 0)
  ZFFT_DETECT_FORM(1, 8, 0)
  ZFFT_DETECT_FORM(4, 8, 0)
  ZFFT_DETECT_FORM(16, 8, 0)
  ZFFT_DETECT_FORM(16, 64, 32)
#undef ZFFT_DETECT_FORM
  return hipErrorInvalidValue;  // a form the chooser does not have
}

}  // namespace zfft
