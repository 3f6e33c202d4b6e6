// resamp_form_sweep.cpp -- stand-alone sweep of the resampler bank's pure host side
// (csrc/zfft_resamp_plan.cpp) over its domain, built with ASan + UBSan by tests/test_resamp_host.py:
// every (K, L, M, T, stride) gets a form whose LDS request is the sum of its parts, the table
// included in the time form, and fits a launch, whose lane tiles cover the K lanes once; for pushes
// at several counts the spans cover every step once, the kernel's own output ranges
// (resamp_span_outs) cover every output exactly once in order, every output's newest step lies in
// its span with i - k >= 0 inside the staged rows, and the grid and p0 are in range; the count is
// the 128-bit formula; outside the domain the chooser refuses.  No HIP, no plan: set_error and the
// Kaiser of windows.cpp (which needs the HIP headers) are stood in for here -- the design's values
// are checked on the library itself in test_resamp_host.py.
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <numeric>
#include <string>
#include <vector>

#include "zfft_resamp_plan.h"

namespace zfft {
void set_error(const std::string &) {}
}  // namespace zfft
extern "C" int zfft_window_values(int32_t, const double *, int32_t length, double *out) {
  for (int i = 0; i < length; ++i) out[i] = 1.0;  // (a boxcar: the sweep checks memory, not values)
  return ZFFT_OK;
}

using namespace zfft;
using u128 = unsigned __int128;

static long g_bad = 0;
static void check(bool ok, const char *what, long long a, long long b, long long c) {
  if (ok) return;
  if (++g_bad <= 20) std::printf("FAIL %s: %lld %lld %lld\n", what, a, b, c);
}

static u128 cdiv(u128 a, uint64_t d) { return a / d + (a % d != 0); }

int main() {
  long keys = 0;
  const uint64_t n0s[] = {0, 1, 3, 249, 250, ((uint64_t)1 << 32) - 100, ((uint64_t)1 << 40) + 3, ((uint64_t)1 << 62) - 1000000,
                          (uint64_t)1 << 62};
  const int64_t pushes[] = {1, 2, 7, 63, 64, 65, 1023, 4097, 20011, 300007, INT32_MAX};
  const int ratios[][2] = {{1, 1}, {1, 2}, {2, 1}, {3, 2}, {3, 4}, {5, 3}, {1, 7}, {16, 25}, {64, 25}, {147, 250},
                           {160, 147}, {1, 4096}, {512, 1}, {511, 4096}, {512, 4095}, {509, 3}};
  for (int K : {1, 2, 3, 5, 7, 8, 9, 16, 17, 63, 64, 65, 70, 1000, 2048})
    for (const auto &r : ratios)
      for (int T : {1, 2, 3, 4, 5, 8, 16, 17, 24, 32, 127, 128}) {
        const int L = r[0], M = r[1];
        const bool fits = L * T <= kResampMaxTable;
        for (int64_t stride : {(int64_t)K, (int64_t)K + 13, kResampMaxStride}) {
          const ResampForm f = choose_resamp(K, L, M, T, stride, stride == K ? ZFFT_RESAMP_F32 : ZFFT_RESAMP_S16);
          ++keys;
          check(f.ok() == fits && resamp_shape_ok(K, L, M, T) == fits, "a form for every shape, none past L T <= 8192", K, L, T);
          if (!f.ok()) continue;
          const bool streams = K >= kResampLanesMin;
          const int table = streams ? 0 : L * f.pitch;
          check(f.kind == (streams ? kResampStreams : kResampTime), "kind", K, L, M);
          check(streams ? f.lanes >= kResampLanesMin && f.lanes <= kResampLanesMax && (f.lanes & (f.lanes - 1)) == 0 &&
                              f.lanes < 2 * K && f.pitch == 0
                        : f.lanes == K && f.pitch >= T && (f.pitch & 1),
                "lanes and pitch of the form", K, f.lanes, f.pitch);
          check(f.lane_tiles * f.lanes >= K && (f.lane_tiles - 1) * f.lanes < K, "lane tiles cover K once", K, f.lanes, f.lane_tiles);
          check(f.halo == T - 1 && f.span >= 1 && f.span <= kResampSpanMax && f.outs == (int)(((int64_t)f.span * L + M - 1) / M),
                "span", T, f.span, f.outs);
          check(f.K == K && f.L == L && f.M == M && f.T == T, "the shape in the form", K, L, M);
          check(f.lds_bytes == 4 * (table + f.lanes * (f.halo + f.span)), "LDS is the sum of its parts", K, T, f.lds_bytes);
          check(f.lds_bytes <= kResampLdsMax, "LDS fits", K, T, f.lds_bytes);
          check((int64_t)f.span * L + (int64_t)(kResampThreads + 1) * M < INT32_MAX, "the kernel's 32-bit positions", f.span, L, M);
          // L > M: the span is cut to the output loop, but never below one step
          check(f.outs <= kResampTileOuts + L, "outputs of a tile", f.span, L, f.outs);
          for (uint64_t n0 : n0s)
            for (int64_t n : pushes) {
              if (n0 + (uint64_t)n > kResampMaxCount) continue;
              const ResampCut c = resamp_cut(f, n0, n);
              check(c.ok(), "a cut for every push", K, (long long)n, L);
              if (!c.ok()) continue;
              const u128 m0 = cdiv((u128)n0 * (uint64_t)L, (uint64_t)M);
              check(c.nspans == (n + f.span - 1) / f.span && c.ntiles == c.nspans * f.lane_tiles, "the spans cover the push", K,
                    (long long)n, f.span);
              check(c.grid >= 1 && c.grid <= kResampGridMax && (c.grid == c.ntiles || c.grid == kResampGridMax), "grid", K,
                    (long long)n, c.grid);
              check(c.p0 >= 0 && c.p0 < M && (u128)c.p0 == m0 * (uint64_t)M - (u128)n0 * (uint64_t)L, "first output", L, M, c.p0);
              check(c.outs == (int64_t)(cdiv(((u128)n0 + (uint64_t)n) * (uint64_t)L, (uint64_t)M) - m0) &&
                        c.outs == resamp_steps(n0, n, L, M),
                    "outputs", L, M, (long long)c.outs);
              if (c.nspans > 256) continue;  // (the walk below span by span, on pushes of moderate length)
              int64_t next = 0;
              for (int64_t b = 0; b < c.nspans; ++b) {
                const int64_t s0 = b * f.span, s1 = s0 + f.span < n ? s0 + f.span : n;
                int64_t j0, j1;
                resamp_span_outs(s0, s1, c.p0, L, M, &j0, &j1);
                check(j0 == next && j1 >= j0 && j1 - j0 <= f.outs, "outputs once and in order", (long long)b, (long long)j0,
                      (long long)next);
                next = j1;
                for (int64_t j : {j0, j1 - 1}) {
                  if (j < j0 || j >= j1) continue;
                  // the kernel's lines: rel on the span's upsampled axis, its row and phase
                  const int64_t rel = c.p0 + j * M - s0 * L;
                  const int i = (int)(rel / L), ph = (int)(rel - (int64_t)i * L);
                  // ... against the rule on the absolute axis, 128 bits wide
                  const u128 u = (m0 + (uint64_t)j) * (uint64_t)M;
                  check(rel >= 0 && rel < (int64_t)f.span * L + M && (u128)(n0 + (uint64_t)s0 + (uint64_t)i) == u / (uint64_t)L &&
                            (u128)ph == u % (uint64_t)L,
                        "position and phase", (long long)b, (long long)j, ph);
                  check(s0 + i >= s0 && s0 + i < s1 && i + f.halo - (T - 1) >= 0 &&
                            4 * (table + f.lanes * (i + f.halo + 1)) <= f.lds_bytes && ph * (streams ? T : f.pitch) + T <= (streams ? L * T : table),
                        "the filter reads inside the rows and the table", (long long)b, (long long)j, i);
                }
              }
              check(next == c.outs, "every output", K, (long long)next, (long long)c.outs);
            }
          for (int64_t n : {(int64_t)0, (int64_t)-1, (int64_t)INT32_MAX + 1})
            check(!resamp_cut(f, 0, n).ok(), "refused steps", K, (long long)n, 0);
          check(!resamp_cut(f, ((uint64_t)1 << 62) + 1, 5).ok(), "refused n0", K, 0, 0);
        }
      }
  // the sum of a cut stream's counts is the whole's
  for (const auto &r : ratios)
    for (uint64_t n0 : n0s) {
      if (n0 + 3000 > kResampMaxCount) continue;
      int64_t sum = 0;
      uint64_t at = n0;
      for (int64_t n : {1, 2, 7, 63, 64, 65, 1023, 775}) sum += resamp_steps(at, n, r[0], r[1]), at += (uint64_t)n;
      check(sum == resamp_steps(n0, (int64_t)(at - n0), r[0], r[1]), "the counts of a cut stream", r[0], r[1], (long long)sum);
    }
  // outside the domain
  for (int K : {0, -1, 2049}) check(!choose_resamp(K, 3, 4, 8, 4096, 0).ok() && !resamp_shape_ok(K, 3, 4, 8), "refused K", K, 0, 0);
  for (int L : {0, -1, 513, 2, 6}) check(!choose_resamp(4, L, 4, 8, 4, 0).ok() && !resamp_shape_ok(4, L, 4, 8), "refused L", L, 0, 0);
  for (int M : {0, -1, 4097, 3, 9}) check(!choose_resamp(4, 3, M, 8, 4, 0).ok() && !resamp_shape_ok(4, 3, M, 8), "refused M", M, 0, 0);
  for (int T : {0, -1, 129}) check(!choose_resamp(4, 3, 4, T, 4, 0).ok() && !resamp_shape_ok(4, 3, 4, T), "refused T", T, 0, 0);
  check(!choose_resamp(4, 3, 4, 8, 3, 0).ok() && !choose_resamp(4, 3, 4, 8, 0, 0).ok() && !choose_resamp(4, 3, 4, 8, -4, 0).ok() &&
            !choose_resamp(4, 3, 4, 8, kResampMaxStride + 1, 0).ok() && !choose_resamp(4, 3, 4, 8, 4, 2).ok() &&
            !choose_resamp(4, 3, 4, 8, 4, -1).ok() && choose_resamp(4, 3, 4, 8, 4, 1).ok(),
        "refused strides and formats", 0, 0, 0);
  check(resamp_steps(0, -1, 3, 4) == 0 && resamp_steps(0, 5, 2, 4) == 0 && resamp_steps(10, 0, 3, 4) == 0 &&
            resamp_steps(((uint64_t)1 << 62) + 1, 5, 3, 4) == 0,
        "refused counts", 0, 0, 0);
  // the design writes exactly L T values
  {
    std::vector<double> h(3 * 11 + 2, -7.0);
    check(zfft_resamp_design(3, 4, 11, 8.0, h.data()) == ZFFT_OK && h[33] == -7.0 && h[32] != -7.0, "the design's length", 33, 0, 0);
    check(zfft_resamp_design(2, 4, 11, 8.0, h.data()) == ZFFT_EINVAL && zfft_resamp_design(512, 1, 17, 8.0, h.data()) == ZFFT_EINVAL &&
              zfft_resamp_design(3, 4, 0, 8.0, h.data()) == ZFFT_EINVAL && zfft_resamp_design(3, 4, 11, -1.0, h.data()) == ZFFT_EINVAL,
          "refused designs", 0, 0, 0);
  }
  if (g_bad) {
    std::printf("resamp_form_sweep: %ld failures over %ld keys\n", g_bad, keys);
    return 1;
  }
  std::printf("resamp_form_sweep: ok (%ld keys)\n", keys);
  return 0;
}
