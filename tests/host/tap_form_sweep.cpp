// tap_form_sweep.cpp -- stand-alone sweep of the channel taps' pure host side
// (csrc/zfft_tap_plan.cpp) over its domain, built with ASan + UBSan by tests/test_tap_host.py:
// every push gets a form whose staging fits the launch's LDS and whose spans cover the push
// exactly once, items whose offsets are the prefix sums of the counts and whose first outputs and
// phase words are the rule's; the counts are the rule's formula; outside the domain it refuses;
// the table and the design write exactly n_taps entries.  No HIP, no plan: the two symbols the
// file takes from the rest of the library (set_error, and the Kaiser of windows.cpp, which needs
// the HIP headers) are stood in for here -- the design's values are checked against scipy in
// test_tap_host.py on the library itself.
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
  const uint64_t n0s[] = {0, 1, 199, 200, 511, 512, 4095, 4096, ((uint64_t)1 << 32) - 100, ((uint64_t)1 << 32) - 1,
                          (uint64_t)1 << 32, ((uint64_t)1 << 32) + 1, ((uint64_t)1 << 40) + 3, (uint64_t)1 << 62};
  const int64_t ns[] = {1, 2, 7, 63, 64, 65, 511, 512, 513, 1023, 2047, 2048, 4095, 4097, 524287, 524288, 524289,
                        1048577, 2097153, 4194304, 4194305, 299008LL * 4096, INT32_MAX};
  const int Ds[] = {1, 2, 3, 7, 8, 31, 32, 33, 64, 200, 511, 512};
  // counts: the formula, and never an output before the tap was opened
  for (uint64_t n0 : n0s)
    for (int64_t n : ns)
      for (int D : Ds)
        for (uint64_t back : {(uint64_t)0, (uint64_t)1, (uint64_t)D, (uint64_t)5000}) {
          if (n0 + (uint64_t)n > kTapMaxCount) continue;
          const uint64_t n_open = back > n0 ? 0 : n0 - back;
          const int64_t c = tap_count(n0, n_open, n, D);
          const uint64_t a = n_open > n0 ? n_open : n0;
          check(c == (int64_t)(cdiv(n0 + (uint64_t)n, (uint64_t)D) - cdiv(a, (uint64_t)D)), "the count's formula",
                (long long)n0, n, D);
          // one rule for every producer: the taps' count is the shared one, and the channeliser's once the tap is open
          check(c == stream_count(n0, n_open, n, D) && c == chan_steps(n0, n, D), "the shared count", (long long)n0, n, D);
          ++keys;
        }
  check(tap_count(10, 50, 20, 4) == 0 && tap_count(10, 29, 20, 4) == 0 && tap_count(10, 28, 20, 4) == 1, "opened late in the push",
        10, 50, 20);
  check(tap_count(0, 0, -1, 4) == 0 && tap_count(0, 0, 5, 0) == 0, "refused counts", 0, 0, 0);

  // forms
  const int lens[] = {1, 2, 65, 257, 1601, 2048};
  for (uint64_t n0 : n0s)
    for (int64_t n : ns)
      for (int max_len : lens)
        for (int ntaps : {0, 1, 4, kTapMaxTaps}) {
          if (n0 + (uint64_t)n > kTapMaxCount) continue;
          std::vector<TapOpen> taps((size_t)ntaps);
          for (int i = 0; i < ntaps; ++i) {
            const int D = Ds[(i * 5 + max_len) % 12], T = 1 + (int)(((int64_t)i * 977 + max_len - 1) % max_len);
            const int64_t fw = (int64_t)((uint64_t)(i + 1) * 0x9E3779B9u % ((uint64_t)1 << 32)) - ((int64_t)1 << 31);
            taps[(size_t)i] = TapOpen{fw, D, i == 0 ? max_len : T, i % 3 ? n0 : n0 / 2, i};
          }
          TapItems items;
          const TapForm f = choose_tap(n0, n, max_len, taps.data(), ntaps, &items);
          ++keys;
          check(f.ok(), "a form for every push", (long long)n0, n, max_len);
          if (!f.ok()) continue;
          check(f.span >= kTapSpanMin && f.span <= kTapSpanMax && (f.span & (f.span - 1)) == 0, "the span", n, f.span, 0);
          check(f.halo == (ntaps ? max_len - 1 : 0), "the halo is the longest filter's", n, f.halo, max_len);
          check(f.pad_shift == kTapNoPad || (f.pad_shift >= kTapPadMin && f.pad_shift <= kTapPadMax), "the pad period", n, f.pad_shift, 0);
          check(f.lds_bytes == (tap_slot(f.halo + f.span - 1, f.pad_shift) + 1) * 8 && f.lds_bytes <= kTapLdsMax,
                "the staging fits the LDS", n, f.lds_bytes, f.span);
          const int64_t spans = (n + f.span - 1) / f.span;
          check(f.first_span >= 0 && f.first_span + (int64_t)f.grid == spans && f.grid >= 1, "the spans reach the push's end once",
                n, f.grid, f.first_span);
          check(ntaps ? f.first_span == 0 : (int64_t)f.first_span * f.span <= (n - (max_len - 1) > 0 ? n - (max_len - 1) : 0),
                "the spans that run hold the next carry (all of them with a tap open)", n, f.first_span, max_len);
          check((f.span == kTapSpanMin || spans >= kTapSpansWanted) &&
                    (f.span == kTapSpanMax || (n + 2 * f.span - 1) / (2 * f.span) < kTapSpansWanted),
                "the largest span that still gives enough workgroups", n, f.span, 0);
          int64_t off = 0;
          for (int i = 0; i < ntaps; ++i) {
            const TapItem &t = items.t[i];
            const TapOpen &o = taps[(size_t)i];
            check(t.out_off == off, "offsets are the prefix sums", n, i, t.out_off);
            check(t.count == tap_count(n0, o.n_open, n, o.D) && t.D == o.D && t.T == o.T && t.slot == i, "the item's tap", n, i, 0);
            check(t.r0 >= 0 && t.r0 < o.D && (n0 + (uint64_t)t.r0) % (uint64_t)o.D == 0, "the first output's sample", n, i, t.r0);
            check(t.r0 + (int64_t)(t.count - 1) * o.D < n && t.r0 + (int64_t)t.count * o.D >= n, "the last output's sample", n, i, t.count);
            const uint64_t fwu = (uint64_t)o.fw & 0xffffffffu;
            check(t.ph0 == (uint32_t)((fwu * ((n0 + (uint64_t)t.r0) & 0xffffffffu)) & 0xffffffffu) &&
                      t.dph == (uint32_t)((fwu * (uint64_t)o.D) & 0xffffffffu),
                  "the phase words", n, i, t.ph0);
            off += t.count;
          }
          check(f.total == off, "the total", n, ntaps, f.total);
        }
  // the layout: one tap of any D gets a staging on which its reads are 2-way at the worst (64 is
  // conflict-free in tap_conflict's units), and no candidate layout models cheaper
  for (int D = 1; D <= kTapMaxDecim; ++D) {
    TapItems items;
    TapOpen t{0, D, 9, 0, 0};
    const TapForm f = choose_tap(0, 100000, 2048, &t, 1, &items);
    const int got = tap_conflict(D, f.pad_shift);
    check(f.ok() && got <= 2 * 64, "at most 2-way for a single tap", D, f.pad_shift, got);
    for (int sh = kTapPadMin; sh <= kTapPadMax; ++sh) check(tap_conflict(D, sh) >= got, "the cheapest layout", D, sh, got);
    check(tap_conflict(D, kTapNoPad) >= got && (D % 2 == 0 || f.pad_shift == kTapNoPad), "odd D: the plain array", D, f.pad_shift, got);
    ++keys;
  }
  // outside the domain
  {
    TapItems items;
    TapOpen t{0, 8, 65, 0, 0};
    check(choose_tap(0, 100, 65, &t, 1, &items).ok(), "a plain push", 0, 0, 0);
    for (int64_t n : {(int64_t)0, (int64_t)-1, (int64_t)INT32_MAX + 1}) check(!choose_tap(0, n, 65, &t, 1, &items).ok(), "refused n", n, 0, 0);
    for (int len : {0, -1, 64, 2049}) check(!choose_tap(0, 100, len, &t, 1, &items).ok(), "refused max_len", len, 0, 0);
    check(!choose_tap(kTapMaxCount + 1, 100, 65, &t, 1, &items).ok(), "refused n0", 0, 0, 0);
    check(!choose_tap(0, 100, 65, &t, kTapMaxTaps + 1, &items).ok() && !choose_tap(0, 100, 65, &t, -1, &items).ok(), "refused ntaps", 0, 0, 0);
    check(!choose_tap(0, 100, 65, nullptr, 1, &items).ok() && !choose_tap(0, 100, 65, &t, 1, nullptr).ok(), "refused null", 0, 0, 0);
    for (int D : {0, -1, 513}) {
      TapOpen b = t;
      b.D = D;
      check(!choose_tap(0, 100, 65, &b, 1, &items).ok(), "refused D", D, 0, 0);
    }
    TapOpen b = t;
    b.n_open = 5;
    check(!choose_tap(0, 100, 65, &b, 1, &items).ok(), "refused a tap opened in the future", 0, 0, 0);
    b = t, b.fw = (int64_t)1 << 31;
    check(!choose_tap(0, 100, 65, &b, 1, &items).ok(), "refused freq_word", 0, 0, 0);
  }
  // the table and the design: exactly n_taps entries, values of the rule
  for (int T : {1, 2, 3, 64, 65, 2048})
    for (int64_t fw : {(int64_t)0, (int64_t)1, (int64_t)-1, -((int64_t)1 << 31), ((int64_t)1 << 31) - 1, (int64_t)0x12345678}) {
      std::vector<float> h((size_t)T), c(2 * (size_t)T + 2, 77.f);
      for (int k = 0; k < T; ++k) h[(size_t)k] = 0.5f + 0.25f * (float)(k % 3);
      check(zfft_tap_table(fw, T, h.data(), c.data()) == ZFFT_OK, "the table builds", T, fw, 0);
      check(c[2 * (size_t)T] == 77.f && c[2 * (size_t)T + 1] == 77.f, "nothing beyond n_taps", T, fw, 0);
      for (int k = 0; k < T; ++k) {
        const double a = 2.0 * M_PI * (double)(((uint64_t)fw & 0xffffffffu) * (uint64_t)k % ((uint64_t)1 << 32)) / 4294967296.0;
        check(std::fabs(c[2 * (size_t)k] - h[(size_t)k] * std::cos(a)) <= 1e-7 && std::fabs(c[2 * (size_t)k + 1] - h[(size_t)k] * std::sin(a)) <= 1e-7,
              "the table's values", T, fw, k);
      }
      std::vector<double> d((size_t)T + 1, 77.0);
      check(zfft_tap_design(T, 0.4 / 8, 8.0, d.data()) == ZFFT_OK && d[(size_t)T] == 77.0, "the design writes n_taps", T, 0, 0);
      double s = 0;
      for (int k = 0; k < T; ++k) s += d[(size_t)k];
      check(std::fabs(s - 1.0) < 1e-12, "unit gain at DC", T, 0, 0);
      ++keys;
    }
  {
    float h = 1.f, c[2];
    double d[4];
    check(zfft_tap_table(0, 0, &h, c) == ZFFT_EINVAL && zfft_tap_table(0, 2049, &h, c) == ZFFT_EINVAL &&
              zfft_tap_table((int64_t)1 << 31, 1, &h, c) == ZFFT_EINVAL && zfft_tap_table(0, 1, nullptr, c) == ZFFT_EINVAL &&
              zfft_tap_table(0, 1, &h, nullptr) == ZFFT_EINVAL,
          "refused tables", 0, 0, 0);
    check(zfft_tap_design(0, 0.1, 8, d) == ZFFT_EINVAL && zfft_tap_design(2049, 0.1, 8, d) == ZFFT_EINVAL &&
              zfft_tap_design(3, 0.0, 8, d) == ZFFT_EINVAL && zfft_tap_design(3, 0.5, 8, d) == ZFFT_EINVAL &&
              zfft_tap_design(3, NAN, 8, d) == ZFFT_EINVAL && zfft_tap_design(3, 0.1, -1, d) == ZFFT_EINVAL &&
              zfft_tap_design(3, 0.1, NAN, d) == ZFFT_EINVAL && zfft_tap_design(3, 0.1, 8, nullptr) == ZFFT_EINVAL,
          "refused designs", 0, 0, 0);
  }
  if (g_bad) {
    std::printf("tap_form_sweep: %ld checks failed over %ld keys\n", g_bad, keys);
    return 1;
  }
  std::printf("tap_form_sweep: ok (%ld keys)\n", keys);
  return 0;
}
