// zfft_demod_plan.h -- how a push of the demodulator bank (demod_kernels.hip; rule in zfft.h,
// zfft_plan_demod) is tiled, as a value: a pure host function of the bank's shape and the two
// strides of the input.  No HIP, no plan: zfft_demod.cpp launches what it returns, and
// tests/test_demod_host.py and tests/host/demod_form_sweep.cpp sweep it without a device.  The
// form does not depend on the push: how a push of `steps` at count n0 falls into the form's tiles
// is demod_cut, beside it (zfft_demod_plan.cpp), with the output counts.
#pragma once

#include <cstddef>
#include <cstdint>

#include "zfft.h"
#include "zfft_stream_plan.h"

namespace zfft {

constexpr int kDemodMaxStreams = 1024;  // K
constexpr int kDemodMaxTaps = 1024;     // Ta
constexpr int kDemodMaxDecim = 64;      // Da
constexpr int kDemodThreads = 256;      // threads of a workgroup (four waves)
constexpr int kDemodLanesMax = 64;      // streams of a tile in the streams form: a wave's width
constexpr int kDemodLanesMin = 8;       // ... and the narrowest: a row of 64 bytes
constexpr int kDemodSpanMax = 8192;     // input steps a tile owns, at most
constexpr int kDemodLdsWant = 40 * 1024;  // bytes of LDS a tile should take: four workgroups a CU
constexpr int kDemodLdsMax = 64 * 1024;   // ... and may take where the history is long (no attribute)
constexpr int kDemodCuLds = 160 * 1024;   // LDS of a CU
constexpr int kDemodPadShift = 5;         // time form: one pad slot after every 32 detected values
constexpr int kDemodGridMax = 1 << 16;    // workgroups of a launch: they walk the tiles round-robin
constexpr int64_t kDemodMaxPush = kStreamMaxPush;        // steps of a push
constexpr uint64_t kDemodMaxCount = kStreamMaxCount;     // the bank's step count (zfft_demod_reset)
constexpr int64_t kDemodMaxStride = (int64_t)1 << 31;   // either stride, in complex samples

enum DemodKind {
  kDemodTime = 0,     // lanes along time: a tile is one stream, consecutive lanes read consecutive steps
  kDemodStreams = 1,  // lanes along streams: a tile is `lanes` neighbouring streams, a lane walks its own LDS column
};

#if defined(__HIPCC__)
#define ZFFT_DEMOD_HD __host__ __device__
#else
#define ZFFT_DEMOD_HD
#endif

// Where detected value i of a tile's column (0 = the first of the history) lives in LDS, in rows:
// the streams form keeps the plain array (a wave reads one row: consecutive banks); in the time
// form the lanes of a wave read Da rows apart, and one pad row after every 32 spreads the even Da
// over the banks again (Da = 64: 2-way instead of 32-way).
ZFFT_DEMOD_HD inline int demod_row(int i, int kind) { return kind == kDemodTime ? i + (i >> kDemodPadShift) : i; }

// The outputs of a push whose step r0 + j Da lies in the span [s0, s1): [*j0, *j1).  (The kernel's
// own arithmetic, here so that the sweep checks the same lines.)
ZFFT_DEMOD_HD inline void demod_span_outs(int64_t s0, int64_t s1, int r0, int Da, int64_t *j0, int64_t *j1) {
  const int64_t d0 = s0 - r0, d1 = s1 - r0;
  *j0 = d0 <= 0 ? 0 : (d0 + Da - 1) / Da;
  *j1 = d1 <= 0 ? 0 : (d1 + Da - 1) / Da;
}

// A tile is `span` input steps of `lanes` streams: span b of the push is the steps [b span, +span),
// stream tile t the streams [t lanes, +lanes).  A workgroup detects the span's samples and the
// `halo` before them once into LDS (column of stream l at [row * lanes + l]) and filters from there.
struct DemodForm {
  int kind = kDemodTime;
  int lanes = 0;         // streams of a tile: 1 (time form) or a power of two in [8, 64]
  int outs = 0;          // output steps of a full span: span / Da
  int span = 0;          // input steps of a tile: outs Da, at most kDemodSpanMax where outs > 1
  int halo = 0;          // Ta - 1 detected values before a span (and one more input sample for FM)
  int lds_bytes = 0;     // 4 lanes (demod_row(halo + span - 1) + 1)
  int stream_tiles = 0;  // ceil(K / lanes)
  bool ok() const { return span > 0; }
};

// How a push falls into a form's tiles.
struct DemodCut {
  int64_t nspans = 0;  // ceil(steps / span)
  int64_t ntiles = 0;  // nspans stream_tiles
  int64_t outs = 0;    // outputs of the push (demod_steps)
  int r0 = 0;          // the push's step of its first output, [0, Da)
  int grid = 0;        // min(ntiles, kDemodGridMax)
  bool ok() const { return grid > 0; }
};

bool demod_shape_ok(int K, int Ta, int Da);
// step_stride in [1, 2^31]; stream_stride in [1, 2^31], or anything in [0, 2^31] for K = 1
bool demod_strides_ok(int K, int64_t step_stride, int64_t stream_stride);

// ceil((n0 + steps) / Da) - ceil(n0 / Da): the outputs of a push of `steps` at count n0 (rule 3).
// 0 outside steps >= 0, Da >= 1, n0 <= 2^62 (stream_count).
inline int64_t demod_steps(uint64_t n0, int64_t steps, int32_t Da) { return stream_count(n0, n0, steps, Da); }

// !ok() outside a valid shape and valid strides.
DemodForm choose_demod(int K, int Ta, int Da, int64_t step_stride, int64_t stream_stride);

// !ok() outside 1 <= steps <= 2^31 - 1, n0 <= 2^62, a form that is ok.
DemodCut demod_cut(const DemodForm &f, uint64_t n0, int64_t steps, int Da);

}  // namespace zfft
