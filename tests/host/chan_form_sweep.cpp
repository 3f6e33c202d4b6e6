// chan_form_sweep.cpp -- stand-alone sweep of the channeliser's pure host side
// (csrc/zfft_chan_plan.cpp) over its domain, built with ASan + UBSan by tests/test_chan_host.py:
// every push of every shape gets a form whose spans are whole steps and cover the push exactly
// once, whose LDS request is the sum of its parts and fits a launch, and whose first step and
// step count are the rule's; the channel positions are a permutation that the transform's passes
// produce; the twiddles are unit vectors; outside the domain the chooser refuses.  No HIP, no
// plan: set_error and the Kaiser of windows.cpp (which needs the HIP headers) are stood in for
// here -- the design's values are checked on the library itself in test_chan_host.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <string>
#include <vector>

#include "zfft_chan_plan.h"
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
  const uint64_t n0s[] = {0, 1, 3, 4, 5, 31, 32, 511, 512, 513, 4095, ((uint64_t)1 << 32) - 100, ((uint64_t)1 << 32) - 1,
                          (uint64_t)1 << 32, ((uint64_t)1 << 40) + 3, ((uint64_t)1 << 62) - INT32_MAX, (uint64_t)1 << 62};
  const int64_t ns[] = {1, 2, 7, 8, 9, 63, 511, 512, 513, 1023, 2047, 2048, 4095, 4097, 65536, 524287, 524288, 524289,
                        2097153, 4194305, 299008LL * 4096, INT32_MAX};
  for (int M = kChanMinM; M <= kChanMaxM; M *= 2) {
    // the positions: a permutation of [0, M), and what the passes make of a one-hot spectrum's index
    std::vector<int> seen((size_t)M, 0);
    for (int c = 0; c < M; ++c) {
      const int pos = chan_position(M, c);
      check(pos >= 0 && pos < M && !seen[(size_t)(pos < 0 || pos >= M ? 0 : pos)]++, "a position twice", M, c, pos);
    }
    std::vector<float> tw((size_t)2 * M + 2, -7.f);
    chan_twiddles(M, tw.data());
    check(tw[(size_t)2 * M] == -7.f && tw[(size_t)2 * M + 1] == -7.f, "twiddles past the table", M, 0, 0);
    check(tw[0] == 1.f && tw[1] == 0.f && tw[(size_t)M / 2] == 0.f && tw[(size_t)M / 2 + 1] == -1.f && tw[(size_t)M] == -1.f &&
              tw[(size_t)M + 1] == 0.f,
          "the quadrants are exact", M, 0, 0);
    for (int i = 0; i < M; ++i) {
      const double a = 2.0 * M_PI * i / M;
      check(std::fabs(tw[2 * i] - std::cos(a)) <= 6e-8 && std::fabs(tw[2 * i + 1] + std::sin(a)) <= 6e-8, "a twiddle", M, i, 0);
    }
    for (int P : {1, 2, 3, 7, 8, 9, 16, kChanMaxLen / M, kChanMaxLen / M + 1})
      for (int D : {M, M / 2, M / 4, M + 1, 0})
        for (int K : {1, 2, M / 2 + 1, M, M + 1})
          for (uint64_t n0 : n0s)
            for (int64_t n : ns) {
              const ChanForm f = choose_chan(n0, n, M, P, D, K);
              const bool in_domain = P >= 1 && P <= kChanMaxLen / M && (D == M || D == M / 2) && K >= 1 && K <= M &&
                                     n0 <= kChanMaxCount;
              check(f.ok() == in_domain, "the domain", M, P, D);
              check(chan_shape_ok(M, P, D) == (P >= 1 && P <= kChanMaxLen / M && (D == M || D == M / 2)), "shape_ok", M, P, D);
              ++keys;
              // one rule for every producer: the steps are the shared count, and a tap's that was open before the push
              check(chan_steps(n0, n, D) == stream_count(n0, n0, n, D) && tap_count(n0, n0 / 2, n, D) == chan_steps(n0, n, D),
                    "the shared count", (long long)n0, n, D);
              if (!f.ok()) continue;
              const int T = M * P;
              check(f.points == 4096 || f.points == 2048 || f.points == 1024, "points", M, P, f.points);
              check(f.steps_per_span * M == f.points && f.span == f.steps_per_span * D && f.span % D == 0, "whole steps", M, D,
                    f.span);
              check(f.halo == T - 1, "halo", M, P, f.halo);
              check(f.kind == (P <= kChanRegTaps ? kChanRegs : kChanLds), "kind", M, P, f.kind);
              check(f.lds_bytes == 8 * (f.halo + f.span + f.points + M) + 4 * K + (f.kind == kChanLds ? 4 * T : 0) &&
                        f.lds_bytes <= kChanLdsMax,
                    "LDS", M, P, f.lds_bytes);
              check(f.nspans == (n + f.span - 1) / f.span && f.nspans >= 1, "the spans cover the push", M, n, f.span);
              check(f.grid >= 1 && f.grid <= kChanGridMax && (f.grid == f.nspans || f.grid == kChanGridMax), "grid", M, n, f.grid);
              int prod = f.radix1;
              for (int i = 1; i < f.passes; ++i) prod *= 4;
              check((f.radix1 == 4 || f.radix1 == 8) && prod == M && f.passes <= kChanMaxPasses, "radices", M, f.radix1, f.passes);
              const uint64_t m0 = cdiv(n0, (uint64_t)D);
              check(f.r0 >= 0 && f.r0 < D && (n0 + (uint64_t)f.r0) % (uint64_t)D == 0, "first step", M, D, f.r0);
              check(f.odd0 == (D != M ? (int)(m0 & 1) : 0), "parity", M, D, f.odd0);
              check(f.steps == (int64_t)(cdiv(n0 + (uint64_t)n, (uint64_t)D) - m0) && f.steps == chan_steps(n0, n, D), "steps", M, D,
                    f.steps);
              // every step lies in the span its index says: step j at sample r0 + j D of span j / steps_per_span
              if (f.steps > 0) {
                const int64_t last = f.r0 + (f.steps - 1) * D;
                check(last < n && last / f.span == (f.steps - 1) / f.steps_per_span && last / f.span < f.nspans, "last step's span",
                      M, n, last);
              }
              // the span grows only when the push is long enough, shrinks only to 1024 points
              if (f.points > kChanPointsMin) check(f.nspans >= kChanSpansWanted, "a long span on a short push", M, n, f.points);
            }
    for (int64_t n : {(int64_t)0, (int64_t)-1, (int64_t)INT32_MAX + 1})
      check(!choose_chan(0, n, M, 1, M, M).ok(), "refused n", M, n, 0);
    check(!choose_chan(((uint64_t)1 << 62) + 1, 5, M, 1, M, M).ok(), "refused n0", M, 0, 0);
    check(!choose_chan(0, 5, M, 1, M, 0).ok(), "refused K", M, 0, 0);
  }
  for (int M : {0, 1, 4, 7, 12, 24, 2048, -8})
    check(!choose_chan(0, 100, M, 1, M, 1).ok() && !chan_shape_ok(M, 1, M), "refused M", M, 0, 0);
  check(chan_steps(0, -1, 4) == 0 && chan_steps(0, 5, 0) == 0 && chan_steps(10, 0, 4) == 0, "refused counts", 0, 0, 0);
  // the design writes exactly M P values
  {
    std::vector<double> h(64 + 2, -7.0);
    check(zfft_chan_design(8, 8, 8.0, h.data()) == ZFFT_OK && h[64] == -7.0 && h[63] != -7.0, "the design's length", 8, 8, 0);
    check(zfft_chan_design(12, 8, 8.0, h.data()) == ZFFT_EINVAL && zfft_chan_design(8, 257, 8.0, h.data()) == ZFFT_EINVAL,
          "refused designs", 0, 0, 0);
  }
  if (g_bad) {
    std::printf("chan_form_sweep: %ld failures over %ld keys\n", g_bad, keys);
    return 1;
  }
  std::printf("chan_form_sweep: ok (%ld keys)\n", keys);
  return 0;
}
