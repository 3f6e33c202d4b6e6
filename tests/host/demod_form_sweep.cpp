// demod_form_sweep.cpp -- stand-alone sweep of the demodulator bank's pure host side
// (csrc/zfft_demod_plan.cpp) over its domain, built with ASan + UBSan by tests/test_demod_host.py:
// every (K, Ta, Da, strides) gets a form whose LDS request is the sum of its parts and fits a
// launch and a CU, whose stream tiles cover the K streams once and whose spans are whole output
// steps; for pushes at several counts the spans cover every step once, the kernel's own output
// ranges (demod_span_outs) cover every output exactly once in order, and every LDS row the filter
// reads lies inside the request; outside the domain the chooser refuses.  No HIP, no plan:
// set_error and the Kaiser of windows.cpp (which needs the HIP headers) are stood in for here --
// the design's values are checked on the library itself in test_demod_host.py.
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <string>
#include <vector>

#include "zfft_chan_plan.h"
#include "zfft_demod_plan.h"
#include "zfft_tap_plan.h"

namespace zfft {
void set_error(const std::string &) {}
}  // namespace zfft
extern "C" int zfft_window_values(int32_t, const double *, int32_t length, double *out) {
  for (int i = 0; i < length; ++i) out[i] = 1.0;  // (a boxcar: the sweep checks memory, not values)
  return ZFFT_OK;
}

using namespace zfft;

static long g_bad = 0;
static void check(bool ok, const char *what, long long a, long long b, long long c) {
  if (ok) return;
  if (++g_bad <= 20) std::printf("FAIL %s: %lld %lld %lld\n", what, a, b, c);
}

static uint64_t cdiv(uint64_t a, uint64_t d) { return a / d + (a % d != 0); }

int main() {
  long keys = 0;
  const uint64_t n0s[] = {0, 1, 3, 63, 64, ((uint64_t)1 << 32) - 100, ((uint64_t)1 << 40) + 3, (uint64_t)1 << 62};
  const int64_t pushes[] = {1, 2, 7, 63, 64, 65, 1023, 4097, 20011, 65536, 300007, INT32_MAX};
  for (int K : {1, 2, 3, 5, 7, 8, 9, 16, 17, 63, 64, 65, 100, 1000, 1024})
    for (int Ta : {1, 2, 3, 4, 5, 8, 17, 33, 65, 256, 513, 1023, 1024})
      for (int Da : {1, 2, 3, 4, 8, 31, 32, 63, 64}) {
        const int64_t strides[][2] = {{K, 1}, {1, 4096}, {1, K > 1 ? 1 : 0}, {7, 3}, {kDemodMaxStride, 1}, {1, kDemodMaxStride},
                                      {2 * (int64_t)K, 1}, {3, 2}};
        for (const auto &st : strides) {
          const DemodForm f = choose_demod(K, Ta, Da, st[0], st[1]);
          ++keys;
          check(f.ok(), "a form for every shape", K, Ta, Da);
          if (!f.ok()) continue;
          const bool streams = st[1] == 1 && K >= kDemodLanesMin;
          check(f.kind == (streams ? kDemodStreams : kDemodTime), "kind", K, st[0], st[1]);
          check(f.lanes >= 1 && f.lanes <= kDemodLanesMax && (f.lanes & (f.lanes - 1)) == 0, "lanes", K, Ta, f.lanes);
          check(streams ? f.lanes >= kDemodLanesMin && f.lanes < 2 * K : f.lanes == 1, "lanes of the form", K, Ta, f.lanes);
          check(f.stream_tiles * f.lanes >= K && (f.stream_tiles - 1) * f.lanes < K, "stream tiles cover K once", K, f.lanes,
                f.stream_tiles);
          check(f.halo == Ta - 1 && f.outs >= 1 && f.span == f.outs * Da && (f.outs == 1 || f.span <= kDemodSpanMax), "span", Ta,
                Da, f.span);
          check(f.lds_bytes == 4 * f.lanes * (demod_row(f.halo + f.span - 1, f.kind) + 1), "LDS is the sum of its parts", K, Ta,
                f.lds_bytes);
          check(f.lds_bytes <= kDemodLdsMax && f.lds_bytes <= kDemodCuLds, "LDS fits", K, Ta, f.lds_bytes);
          // the long budget only where the short one would detect every sample more than twice
          if (f.lds_bytes > kDemodLdsWant) check(f.lanes == (streams ? kDemodLanesMin : 1), "the long budget", K, Ta, f.lanes);
          for (uint64_t n0 : n0s)
            for (int64_t n : pushes) {
              const DemodCut c = demod_cut(f, n0, n, Da);
              check(c.ok(), "a cut for every push", K, (long long)n, Da);
              if (!c.ok()) continue;
              const uint64_t m0 = cdiv(n0, (uint64_t)Da);
              check(c.nspans == (n + f.span - 1) / f.span && c.ntiles == c.nspans * f.stream_tiles, "the spans cover the push", K,
                    (long long)n, f.span);
              check(c.grid >= 1 && c.grid <= kDemodGridMax && (c.grid == c.ntiles || c.grid == kDemodGridMax), "grid", K,
                    (long long)n, c.grid);
              check(c.r0 >= 0 && c.r0 < Da && (n0 + (uint64_t)c.r0) % (uint64_t)Da == 0, "first output", K, Da, c.r0);
              check(c.outs == (int64_t)(cdiv(n0 + (uint64_t)n, (uint64_t)Da) - m0) && c.outs == demod_steps(n0, n, Da), "outputs", K, Da,
                    (long long)c.outs);
              // one rule for every producer: the outputs are the shared count, and a tap's that was open before the push
              check(demod_steps(n0, n, Da) == stream_count(n0, n0, n, Da) && tap_count(n0, n0 / 2, n, Da) == chan_steps(n0, n, Da),
                    "the shared count", (long long)n0, (long long)n, Da);
              if (c.nspans > 512) continue;  // (the walk below span by span, on pushes of moderate length)
              int64_t next = 0;
              for (int64_t b = 0; b < c.nspans; ++b) {
                const int64_t s0 = b * f.span, s1 = s0 + f.span < n ? s0 + f.span : n;
                int64_t j0, j1;
                demod_span_outs(s0, s1, c.r0, Da, &j0, &j1);
                check(j0 == next && j1 >= j0 && j1 - j0 <= f.outs, "outputs once and in order", (long long)b, (long long)j0,
                      (long long)next);
                next = j1;
                for (int64_t j : {j0, j1 - 1}) {
                  if (j < j0 || j >= j1) continue;
                  const int64_t at = c.r0 + j * Da;
                  const int i0 = (int)(at - s0) + f.halo;
                  check(at >= s0 && at < s1 && i0 - (Ta - 1) >= 0 &&
                            4 * f.lanes * (demod_row(i0, f.kind) + 1) <= f.lds_bytes,
                        "the filter reads inside the column", (long long)b, (long long)j, i0);
                }
              }
              check(next == c.outs, "every output", K, (long long)next, (long long)c.outs);
            }
          for (int64_t n : {(int64_t)0, (int64_t)-1, (int64_t)INT32_MAX + 1})
            check(!demod_cut(f, 0, n, Da).ok(), "refused steps", K, (long long)n, 0);
          check(!demod_cut(f, ((uint64_t)1 << 62) + 1, 5, Da).ok(), "refused n0", K, 0, 0);
        }
      }
  // outside the domain
  for (int K : {0, -1, 1025}) check(!choose_demod(K, 8, 2, 1, 1).ok() && !demod_shape_ok(K, 8, 2), "refused K", K, 0, 0);
  for (int Ta : {0, -1, 1025}) check(!choose_demod(4, Ta, 2, 4, 1).ok() && !demod_shape_ok(4, Ta, 2), "refused Ta", Ta, 0, 0);
  for (int Da : {0, -1, 65}) check(!choose_demod(4, 8, Da, 4, 1).ok() && !demod_shape_ok(4, 8, Da), "refused Da", Da, 0, 0);
  check(!choose_demod(4, 8, 2, 0, 1).ok() && !choose_demod(4, 8, 2, 4, 0).ok() && !choose_demod(4, 8, 2, -4, 1).ok() &&
            !choose_demod(4, 8, 2, 4, -1).ok() && !choose_demod(4, 8, 2, kDemodMaxStride + 1, 1).ok() &&
            !choose_demod(1, 8, 2, 1, -1).ok() && choose_demod(1, 8, 2, 1, 0).ok(),
        "refused strides", 0, 0, 0);
  check(demod_steps(0, -1, 4) == 0 && demod_steps(0, 5, 0) == 0 && demod_steps(10, 0, 4) == 0, "refused counts", 0, 0, 0);
  // the design writes exactly n_taps values
  {
    std::vector<double> h(33 + 2, -7.0);
    check(zfft_demod_design(33, 0.1, 8.0, h.data()) == ZFFT_OK && h[33] == -7.0 && h[32] != -7.0, "the design's length", 33, 0, 0);
    check(zfft_demod_design(0, 0.1, 8.0, h.data()) == ZFFT_EINVAL && zfft_demod_design(1025, 0.1, 8.0, h.data()) == ZFFT_EINVAL,
          "refused designs", 0, 0, 0);
  }
  if (g_bad) {
    std::printf("demod_form_sweep: %ld failures over %ld keys\n", g_bad, keys);
    return 1;
  }
  std::printf("demod_form_sweep: ok (%ld keys)\n", keys);
  return 0;
}
