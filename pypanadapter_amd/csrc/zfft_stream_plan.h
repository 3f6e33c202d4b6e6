// zfft_stream_plan.h -- the counting rule every producer on a sample stream shares (the channel
// taps, the channeliser, the demodulator bank): a consumer that decimates by D has its outputs at
// the units m D of the stream, so what a push gives depends on the stream's count alone.  Pure
// and header-only, no HIP: the three *_plan.cpp files and their stand-alone sweeps include it.
#pragma once

#include <algorithm>
#include <cstdint>

namespace zfft {

constexpr int64_t kStreamMaxPush = INT32_MAX;            // units (samples or steps) of a push
constexpr uint64_t kStreamMaxCount = (uint64_t)1 << 62;  // a stream's count (the *_reset calls)

inline uint64_t ceil_div(uint64_t a, uint64_t d) { return a / d + (a % d != 0); }

// ceil((n0 + n) / D) - ceil(max(n0, n_open) / D): the outputs of a push of n units at count n0
// for a consumer opened at count n_open.  0 outside 0 <= n <= 2^31 - 1, D >= 1, n0 <= 2^62.
inline int64_t stream_count(uint64_t n0, uint64_t n_open, int64_t n, int32_t D) {
  if (n < 0 || D < 1 || n0 > kStreamMaxCount || n > kStreamMaxPush) return 0;
  const uint64_t a = std::max(n0, n_open), end = n0 + (uint64_t)n;
  if (a >= end) return 0;
  return (int64_t)(ceil_div(end, (uint64_t)D) - ceil_div(a, (uint64_t)D));
}

// The unit of a push at count n0 that gives the first output, [0, D): the next m D from n0 on.
inline uint64_t stream_first(uint64_t n0, int32_t D) { return ceil_div(n0, (uint64_t)D) * (uint64_t)D - n0; }

}  // namespace zfft
