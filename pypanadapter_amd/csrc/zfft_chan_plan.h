// zfft_chan_plan.h -- how a push of the channeliser (chan_kernels.hip; rule in zfft.h,
// zfft_plan_chan) is cut, as a value: a pure host function of the plan's sample count, the samples
// of the call and the bank's shape.  No HIP, no plan: zfft_chan.cpp launches what it returns, and
// tests/test_chan_host.py and tests/host/chan_form_sweep.cpp sweep it without a device.  The other
// pure pieces live beside it (zfft_chan_plan.cpp): the step counts, the transform's radices, the
// twiddle table and where a channel ends up in the transform's buffer.
#pragma once

#include <cstddef>
#include <cstdint>

#include "zfft.h"
#include "zfft_stream_plan.h"

namespace zfft {

constexpr int kChanMinM = 8, kChanMaxM = 1024;  // channels: a power of two
constexpr int kChanMaxLen = 2048;               // M P, the prototype's taps, at most
constexpr int kChanThreads = 256;               // threads of a workgroup (four waves)
constexpr int kChanPointsMax = 4096;            // transform points (steps x M) a span holds, at most ...
constexpr int kChanPointsMin = 1024;            // ... and at least (one step of the largest M)
constexpr int kChanSpansWanted = 512;           // spans a push should give before the span grows
constexpr int kChanGridMax = 1024;              // workgroups of a launch: they walk the spans round-robin
constexpr int kChanLdsMax = 64 * 1024;          // bytes of LDS a launch may ask for without an attribute
constexpr int kChanRegTaps = 8;                 // P up to here: a lane keeps its coefficients in registers
constexpr int kChanMaxPasses = 5;               // log4(1024)
constexpr int64_t kChanMaxPush = kStreamMaxPush;      // samples of a push
constexpr uint64_t kChanMaxCount = kStreamMaxCount;   // the plan's sample count (zfft_chan_reset)

enum ChanKind {
  kChanRegs = 0,  // P <= kChanRegTaps: the R1 P coefficients of a lane's branches live in registers
  kChanLds = 1,   // longer branches: the prototype is staged in LDS once per workgroup
};

// One launch: span b < nspans is the samples [b span, +span) of the push and the `steps_per_span`
// steps in it; a workgroup stages a span behind `halo` earlier samples (from the carry where they
// precede the push) and transforms its steps in `points` complex64 of LDS.  Workgroup g takes the
// spans g, g + grid, ...
struct ChanForm {
  int span = 0;            // samples per span: steps_per_span D
  int steps_per_span = 0;  // points / M
  int points = 0;          // 4096, 2048 or 1024
  int halo = 0;            // M P - 1
  int kind = kChanRegs;
  int radix1 = 0;          // the first pass's radix, fused with the FIR: 8 where log2 M is odd, else 4
  int passes = 0;          // the first pass and the radix-4 passes after it
  int lds_bytes = 0;       // 8 (halo + span + points + M) + 4 K (+ 4 M P when kind = kChanLds)
  int grid = 0;            // min(nspans, kChanGridMax)
  int r0 = 0;              // the push's sample of its first step, [0, D)
  int odd0 = 0;            // D = M / 2: the first step's m is odd
  int64_t nspans = 0;      // ceil(n / span)
  int64_t steps = 0;       // steps of the push
  bool ok() const { return span > 0; }
};

bool chan_shape_ok(int M, int P, int D);

// ceil((n0 + n) / D) - ceil(n0 / D): the steps of a push of n samples at count n0 (the rule's
// item 4; the count starts at the reset value, so n_start <= n0: stream_count).  0 outside n >= 0, D >= 1.
inline int64_t chan_steps(uint64_t n0, int64_t n, int32_t D) { return stream_count(n0, n0, n, D); }

// The form of a push of n samples at count n0 with K kept channels.  !ok() outside 1 <= n <= 2^31 - 1,
// n0 <= 2^62, a valid shape, 1 <= K <= M.
ChanForm choose_chan(uint64_t n0, int64_t n, int M, int P, int D, int K);

// The transform is a decimation-in-frequency FFT in place: pass 1 has radix radix1 on length M,
// the others radix 4 on the lengths M / radix1, M / (4 radix1), ...  Channel c ends at this index
// of a step's M points (the mixed-radix digit reversal).
int chan_position(int M, int c);

// W_M^i = exp(-2 pi i / M), i < M, each component rounded once from float64; tw_out = 2 M floats.
void chan_twiddles(int M, float *tw_out);

}  // namespace zfft
