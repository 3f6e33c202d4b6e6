// zfft_chan_plan.cpp -- the pure host side of the channeliser (zfft_chan_plan.h): choose_chan, the
// step counts, the transform's layout and twiddles, the default prototype.  No HIP: built into
// libzfft.so and, stand-alone under ASan + UBSan, into tests/host/chan_form_sweep.cpp (which
// supplies set_error and links zfft_tap_plan.cpp and windows.cpp for the design).
#include "zfft_chan_plan.h"

#include <algorithm>
#include <cmath>
#include <string>

namespace zfft {

void set_error(const std::string &msg);  // zfft_plan.cpp

namespace {

int log2i(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

}  // namespace

bool chan_shape_ok(int M, int P, int D) {
  return M >= kChanMinM && M <= kChanMaxM && (M & (M - 1)) == 0 && P >= 1 && P <= kChanMaxLen / M &&
         (D == M || D == M / 2);
}

ChanForm choose_chan(uint64_t n0, int64_t n, int M, int P, int D, int K) {
  ChanForm f;
  if (n < 1 || n > kChanMaxPush || n0 > kChanMaxCount || !chan_shape_ok(M, P, D) || K < 1 || K > M) return f;
  const int T = M * P;
  f.halo = T - 1;
  f.kind = P <= kChanRegTaps ? kChanRegs : kChanLds;
  f.radix1 = (log2i(M) & 1) ? 8 : 4;
  f.passes = 1 + log2i(M / f.radix1) / 2;
  auto lds_of = [&](int points) {
    const int span = points / M * D;
    return 8 * (f.halo + span + points + M) + 4 * K + (f.kind == kChanLds ? 4 * T : 0);
  };
  // the largest span that fits (two workgroups a CU: no request above 64 KB) ...
  int points = kChanPointsMax;
  while (points > kChanPointsMin && lds_of(points) > kChanLdsMax) points /= 2;
  if (lds_of(points) > kChanLdsMax) return f;
  // ... and a shorter one while the push would leave most of the chip idle
  auto spans_of = [&](int pts) { return (n + (int64_t)(pts / M) * D - 1) / ((int64_t)(pts / M) * D); };
  while (points > kChanPointsMin && spans_of(points) < kChanSpansWanted) points /= 2;
  f.points = points;
  f.steps_per_span = points / M;
  f.lds_bytes = lds_of(points);
  f.nspans = spans_of(points);
  f.grid = (int)std::min<int64_t>(f.nspans, kChanGridMax);
  f.r0 = (int)stream_first(n0, D);
  const uint64_t m0 = (n0 + (uint64_t)f.r0) / (uint64_t)D;  // the first step's m
  f.odd0 = D != M ? (int)(m0 & 1) : 0;
  f.steps = chan_steps(n0, n, D);
  f.span = f.steps_per_span * D;
  return f;
}

int chan_position(int M, int c) {
  int L = M, pos = 0, r = (log2i(M) & 1) ? 8 : 4;
  while (L > 1) {
    L /= r;
    pos += (c % r) * L;
    c /= r;
    r = 4;
  }
  return pos;
}

void chan_twiddles(int M, float *tw_out) {
  for (int i = 0; i < M; ++i) {
    // the quadrant exactly, the rest in float64 (|angle| <= pi / 4 would gain nothing here: the
    // float64 error, 1e-16, is far below half a float32 ulp)
    const int q = M / 4, quad = i / q, j = i % q;
    const double a = 2.0 * M_PI * (double)j / (double)M;
    double c = j ? std::cos(a) : 1.0, s = j ? std::sin(a) : 0.0;  // exp(-i a) = (c, -s)
    for (int t = 0; t < quad; ++t) {  // times -i: (c, -s) -> (-s, -c)
      const double c2 = -s, s2 = c;
      c = c2, s = s2;
    }
    tw_out[2 * i] = (float)c;
    tw_out[2 * i + 1] = (float)-s;
  }
}

}  // namespace zfft

using namespace zfft;

// Test hooks (not part of include/zfft.h; no plan, no device): the step count, and the form of a
// push -- form13 = {span, steps_per_span, points, halo, kind, radix1, passes, lds_bytes, grid, r0,
// odd0, nspans, steps}; the position of a channel in the transform's buffer.
extern "C" int64_t zfft__chan_steps(uint64_t n0, int64_t n, int32_t D) { return chan_steps(n0, n, D); }
extern "C" int zfft__chan_form(uint64_t n0, int64_t n, int32_t M, int32_t P, int32_t D, int32_t K, int64_t *form13) {
  if (!form13) return -1;
  const ChanForm f = choose_chan(n0, n, M, P, D, K);
  if (!f.ok()) return -1;
  const int64_t v[13] = {f.span, f.steps_per_span, f.points, f.halo, f.kind, f.radix1, f.passes,
                         f.lds_bytes, f.grid, f.r0, f.odd0, f.nspans, f.steps};
  std::copy(v, v + 13, form13);
  return 0;
}
extern "C" int zfft__chan_position(int32_t M, int32_t c) {
  return M >= kChanMinM && M <= kChanMaxM && (M & (M - 1)) == 0 && c >= 0 && c < M ? chan_position(M, c) : -1;
}

extern "C" int zfft_chan_design(int32_t n_chan, int32_t taps_per_chan, double beta, double *h_out) {
  if (!chan_shape_ok(n_chan, taps_per_chan, n_chan)) {
    set_error("chan_design: n_chan a power of two in [8, 1024], taps_per_chan >= 1, n_chan taps_per_chan <= 2048");
    return ZFFT_EINVAL;
  }
  return zfft_tap_design(n_chan * taps_per_chan, 0.5 / n_chan, beta, h_out);
}
