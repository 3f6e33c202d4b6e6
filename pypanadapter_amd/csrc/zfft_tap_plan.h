// zfft_tap_plan.h -- how a push of the channel taps (tap_kernels.hip; rule in zfft.h,
// zfft_plan_taps) is cut, as a value: a pure host function of the plan's sample count, the
// samples of the call and the open taps.  No HIP, no plan: zfft_tap.cpp launches what it returns,
// and tests/test_tap_host.py and tests/host/tap_form_sweep.cpp sweep it without a device.  The
// other pure pieces of the rule live beside it (zfft_tap_plan.cpp): the output counts, the
// Kaiser design and the modulated table.
#pragma once

#include <cstddef>
#include <cstdint>

#include "zfft.h"
#include "zfft_stream_plan.h"

namespace zfft {

constexpr int kTapMaxTaps = 64;       // slots of a plan, at most
constexpr int kTapMaxLen = 2048;      // taps of a filter, at most
constexpr int kTapMaxDecim = 512;
constexpr int kTapThreads = 256;      // threads of a workgroup (four waves)
constexpr int kTapSpanMax = 4096;     // input samples a workgroup owns, at most ...
constexpr int kTapSpanMin = 512;      // ... and at least (a short push spreads over more of the chip)
constexpr int kTapSpansWanted = 1024; // workgroups a push should give before the span grows
constexpr int kTapLdsMax = 64 * 1024; // bytes of LDS a launch may ask for without an attribute
constexpr int64_t kTapMaxPush = kStreamMaxPush;       // samples of a push
constexpr uint64_t kTapMaxCount = kStreamMaxCount;    // the plan's sample count (zfft_tap_reset)

#if defined(__HIPCC__)
#define ZFFT_TAP_HD __host__ __device__
#else
#define ZFFT_TAP_HD
#endif

// Where staged sample i (0 = the first of the halo) lives in LDS, in complex64 slots: one pad
// slot after every 2^shift samples; shift = kTapNoPad is the plain array.  The lanes of a wave
// read D samples apart: on the plain array that is conflict-free for odd D and gcd(D, 32)-way
// otherwise, and a pad every 2^shift moves each block by one bank pair, which spreads the
// D = 2^shift multiples again -- but costs the odd D near a multiple of 2^shift.  No one layout
// serves every D, so the chooser picks the shift per push from the open taps.
constexpr int kTapNoPad = 31, kTapPadMin = 3, kTapPadMax = 9;
constexpr int kTapLayouts = 8;
constexpr int kTapLayoutShifts[kTapLayouts] = {kTapNoPad, 3, 4, 5, 6, 7, 8, 9};  // the chooser's candidates
ZFFT_TAP_HD inline int tap_slot(int i, int shift) { return i + (i >> shift); }
// The modelled cost of a wave's ds_read_b64 at stride D under `shift`: the bank conflict degree
// of 32 lanes (a half wave; the bank pair of slot s is s mod 32), summed over 64 (k, offset)
// positions; 64 = conflict-free.
int tap_conflict(int D, int shift);
// tap_conflict of every (D, candidate) as [D * kTapLayouts + c], D <= 512: built on the first call
// (about 10^7 operations; zfft_plan_taps makes it, so no push ever does).
const int *tap_conflict_model();

// An open tap as the chooser sees it.
struct TapOpen {
  int64_t fw;       // freq_word, [-2^31, 2^31)
  int32_t D, T;     // decimation, taps
  uint64_t n_open;  // the plan's count when it was opened
  int32_t slot;
};

// An open tap in one push, as the kernel takes it: its output j < count is the sample r0 + j D of
// the push (relative to the push's first sample), rotated by the phase word ph0 + j dph (mod 2^32),
// written to out[out_off + j].
struct TapItem {
  int64_t r0;
  int64_t out_off;
  uint32_t ph0, dph;
  int32_t D, T, slot, count;
};
static_assert(sizeof(TapItem) == 40, "TapItem is 40 bytes");

struct TapItems {
  TapItem t[kTapMaxTaps];
};

// One launch: workgroup g owns the samples [(first_span + g) span, +span) of the push and stages
// them behind `halo` earlier ones (from the carry where they precede the push).
struct TapForm {
  int span = 0;        // samples per workgroup: 512, 1024, 2048 or 4096
  int halo = 0;        // max T - 1 over the open taps
  int pad_shift = kTapNoPad;  // the staging's layout (tap_slot): the cheapest for the open taps, T / D weighted
  int lds_bytes = 0;   // (tap_slot(halo + span - 1, pad_shift) + 1) * 8
  int first_span = 0;  // with no tap open only the spans that reach the next carry run
  int grid = 0;        // workgroups
  int ntaps = 0;
  int64_t total = 0;   // outputs of the push, all taps
  bool ok() const { return span > 0; }
};

// ceil((n0 + n) / D) - ceil(max(n0, n_open) / D): the outputs of a tap in a push of n samples at
// count n0 (the rule's clause on counts; stream_count).  0 outside n >= 0, D >= 1.
inline int64_t tap_count(uint64_t n0, uint64_t n_open, int64_t n, int32_t D) { return stream_count(n0, n_open, n, D); }

// The form of a push of n samples at count n0 on a plan of max_len, and the items of its open
// taps (slot order as given; offsets the prefix sums of the counts).  !ok() outside 1 <= n <= 2^31 - 1,
// n0 <= 2^62, 1 <= max_len <= 2048, 0 <= ntaps <= 64, 1 <= D <= 512, 1 <= T <= max_len,
// n_open <= n0.  layout: 0 = the chooser's pad_shift, else that shift (kTapNoPad or 3 .. 9; the
// measurement hook zfft__plan_tap_layout).
TapForm choose_tap(uint64_t n0, int64_t n, int max_len, const TapOpen *taps, int ntaps, TapItems *items,
                   int layout = 0);

// zfft_tap_design's formula at any length T >= 1 (the resampler's prototype has up to 8192 taps):
// the symmetric Kaiser sinc of unit sum.  The caller has checked 0 < cutoff < 0.5 and beta >= 0.
int kaiser_sinc(int T, double cutoff, double beta, double *h_out);

}  // namespace zfft
