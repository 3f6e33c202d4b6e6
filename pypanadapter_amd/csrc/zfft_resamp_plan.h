// zfft_resamp_plan.h -- how a push of the resampler bank (resamp_kernels.hip; rule in zfft.h,
// zfft_plan_resamp) is tiled, as a value: a pure host function of the bank's shape.  No HIP, no
// plan: zfft_resamp.cpp launches what it returns, and tests/test_resamp_host.py and
// tests/host/resamp_form_sweep.cpp sweep it without a device.  The form does not depend on the
// push: how a push of `steps` at count n0 falls into the form's tiles is resamp_cut, beside it
// (zfft_resamp_plan.cpp), with the output count, whose products pass 2^64.
#pragma once

#include <cstddef>
#include <cstdint>

#include "zfft.h"
#include "zfft_stream_plan.h"

namespace zfft {

constexpr int kResampMaxLanes = 2048;     // K
constexpr int kResampMaxL = 512;          // outputs per M inputs
constexpr int kResampMaxM = 4096;
constexpr int kResampMaxT = 128;          // taps per phase
constexpr int kResampMaxTable = 8192;     // L T, the prototype's length
constexpr int kResampThreads = 256;       // threads of a workgroup (four waves)
constexpr int kResampLanesMax = 64;       // lanes of a tile in the streams form: a wave's width
constexpr int kResampLanesMin = 8;        // ... and the narrowest: a row of 32 bytes
constexpr int kResampSpanMax = 8192;      // input steps a tile owns, at most
constexpr int kResampTileOuts = 4096;     // outputs per lane a tile should give at most (L > M: the span shrinks)
constexpr int kResampLdsWant = 40 * 1024; // bytes of LDS a tile should take: four workgroups a CU
constexpr int kResampLdsMax = 64 * 1024;  // ... and may take (no attribute)
constexpr int kResampGridMax = 1 << 16;   // workgroups of a launch: they walk the tiles round-robin
constexpr int64_t kResampMaxPush = kStreamMaxPush;       // steps of a push
constexpr uint64_t kResampMaxCount = kStreamMaxCount;    // the bank's step count (zfft_resamp_reset)
constexpr int64_t kResampMaxStride = (int64_t)1 << 31;   // step_stride, in floats

enum ResampKind {
  kResampTime = 0,     // K < 8: a tile is a span of all K lanes, the threads run along its outputs
  kResampStreams = 1,  // K >= 8: a tile is `lanes` neighbouring lanes, a thread walks its own LDS column
};

#if defined(__HIPCC__)
#define ZFFT_RESAMP_HD __host__ __device__
#else
#define ZFFT_RESAMP_HD
#endif

// Output j of a push is at p0 + j M on the push's upsampled axis: it reads up to the relative
// step (p0 + j M) / L at phase (p0 + j M) mod L.  The outputs whose newest step lies in the span
// [s0, s1) of the push, s0 L <= p0 + j M < s1 L: [*j0, *j1).  (The kernel's own arithmetic, here
// so that the sweep checks the same lines.  s1 L < 2^40.)
ZFFT_RESAMP_HD inline void resamp_span_outs(int64_t s0, int64_t s1, int p0, int L, int M, int64_t *j0, int64_t *j1) {
  const int64_t d0 = s0 * L - p0, d1 = s1 * L - p0;
  *j0 = d0 <= 0 ? 0 : (d0 + M - 1) / M;
  *j1 = d1 <= 0 ? 0 : (d1 + M - 1) / M;
}

// A tile is `span` input steps of `lanes` lanes: span b of the push is the steps [b span, +span),
// lane tile t the lanes [t lanes, +lanes).  A workgroup stages the span's samples and the `halo`
// before them once into LDS (lane l of row i at [i * lanes + l]) and filters from there; the time
// form keeps the coefficient table beside them, phase-major with rows of `pitch` floats.
struct ResampForm {
  int kind = kResampTime;
  int K = 0, L = 0, M = 0, T = 0;
  int lanes = 0;       // lanes of a tile: K (time form) or a power of two in [8, 64]
  int span = 0;        // input steps of a tile
  int halo = 0;        // T - 1 steps before a span
  int outs = 0;        // outputs of a span, at most: ceil(span L / M)
  int pitch = 0;       // floats of a table row in LDS: T | 1 (time form), 0 (streams form: no table in LDS)
  int lds_bytes = 0;   // 4 (L pitch + lanes (halo + span))
  int lane_tiles = 0;  // ceil(K / lanes)
  bool ok() const { return span > 0; }
};

// How a push falls into a form's tiles.
struct ResampCut {
  int64_t nspans = 0;  // ceil(steps / span)
  int64_t ntiles = 0;  // nspans lane_tiles
  int64_t outs = 0;    // outputs of the push (resamp_steps)
  int p0 = 0;          // the first output on the push's upsampled axis, [0, M)
  int grid = 0;        // min(ntiles, kResampGridMax)
  bool ok() const { return grid > 0; }
};

// 1 <= K <= 2048, 1 <= L <= 512, 1 <= M <= 4096, gcd(L, M) = 1, 1 <= T <= 128, L T <= 8192
bool resamp_shape_ok(int K, int L, int M, int T);
// step_stride in [K, 2^31]
bool resamp_stride_ok(int K, int64_t step_stride);

// ceil((n0 + steps) L / M) - ceil(n0 L / M): the outputs of a push of `steps` at count n0 (rule 3),
// in 128-bit arithmetic: n0 L reaches 2^71.  0 outside 0 <= steps <= 2^31 - 1, n0 <= 2^62, a valid ratio.
int64_t resamp_steps(uint64_t n0, int64_t steps, int L, int M);
// ceil(n0 L / M) M - n0 L, in [0, M): where the push's first output lies on its upsampled axis.
int resamp_p0(uint64_t n0, int L, int M);

// !ok() outside a valid shape, stride and format.
ResampForm choose_resamp(int K, int L, int M, int T, int64_t step_stride, int format);

// !ok() outside 1 <= steps <= 2^31 - 1, n0 <= 2^62, a form that is ok.
ResampCut resamp_cut(const ResampForm &f, uint64_t n0, int64_t steps);

}  // namespace zfft
