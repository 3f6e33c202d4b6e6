// zfft_level_plan.h -- how a push of the level bank (level_kernels.hip; rule in zfft.h,
// zfft_plan_level) is tiled, as a value: a pure host function of the bank's shape.  No HIP, no
// plan: zfft_level.cpp launches what it returns, and tests/test_level_host.py and
// tests/host/level_form_sweep.cpp sweep it without a device.  The form does not depend on the
// push: how a push of `steps` at count n0 of a bank started at n_r falls onto the block grid and
// into the form's tiles is level_cut, beside it (zfft_level_plan.cpp), with emitted().
#pragma once

#include <cstddef>
#include <cstdint>

#include "zfft.h"
#include "zfft_stream_plan.h"

namespace zfft {

constexpr int kLevelMaxLanes = 2048;     // K
constexpr int kLevelMinBlock = 8;        // B, a power of two
constexpr int kLevelMaxBlock = 1024;
constexpr int kLevelMaxHold = 4096;      // H, in blocks
constexpr int kLevelThreads = 256;       // threads of a workgroup (four waves)
constexpr int kLevelLanesMax = 64;       // lanes of a tile in the streams form: a wave's width
constexpr int kLevelLanesMin = 8;        // ... and the narrowest: a row of 32 bytes
constexpr int kLevelTileRows = 256;      // steps of a tile of the peaks and apply kernels, at least (B where B is longer)
constexpr int kLevelGainRowsMax = 1024;  // blocks whose gains a tile of the gains kernel forms, at most
constexpr int kLevelLdsMax = 64 * 1024;  // bytes of LDS a tile may take (no attribute)
constexpr int kLevelGridMax = 1 << 12;   // workgroups of a launch: they walk the tiles round-robin
constexpr int64_t kLevelMaxPush = kStreamMaxPush;       // steps of a push
constexpr uint64_t kLevelMaxCount = kStreamMaxCount;    // the bank's step count (zfft_level_reset)
constexpr int64_t kLevelMaxStride = (int64_t)1 << 31;   // step_stride and key_stride, in floats
constexpr float kLevelCap = 0x1p60f;     // rule 3's cap, and the parameters' upper limit
constexpr float kLevelMin = 0x1p-60f;    // the parameters' lower limit

enum LevelKind {
  kLevelTime = 0,     // K < 8: a tile is a span of all K lanes, the threads run along time
  kLevelStreams = 1,  // K >= 8: a tile is `lanes` neighbouring lanes, a thread stays on its lane
};

#if defined(__HIPCC__)
#define ZFFT_LEVEL_HD __host__ __device__
#else
#define ZFFT_LEVEL_HD
#endif

// Rule 3's m(v): 0 for a NaN, else min(|v|, 2^60).
ZFFT_LEVEL_HD inline float level_mag(float v) {
  const float a = v < 0.f ? -v : v;
  return v != v ? 0.f : (a < kLevelCap ? a : kLevelCap);
}

// Rule 4's block gain of an envelope E >= 0 (never a NaN): the device's arithmetic and the
// meter's on the host, the same lines.  The division is IEEE's, rounded once.
ZFFT_LEVEL_HD inline float level_gain(float E, float target, float gmax, float floor, float squelch) {
  if (squelch > 0.f && E < squelch) return 0.f;
  const float g = target / (E > floor ? E : floor);
  return g < gmax ? g : gmax;
}

// The three kernels of a push work on one axis u >= 0: u = 0 is the first step of the block two
// before the one the count n0 lies in, so that block q of a push is the steps [q B, (q + 1) B) of
// it, the push's first step sits at u_in0 = 2 B + n0 mod B and every carried step at u >= B.
//
// Peaks and apply kernels: a tile is `rows` steps (whole blocks, aligned to the block grid) of
// `lanes` lanes.  Streams form: thread t is lane t mod lanes of row group t / lanes; a row group
// takes `chunk` consecutive steps of the tile, as chunk / piece pieces of `piece` steps that lie
// in one block each, so that a block's gains are formed once a piece and a block's peak is the
// max of B / piece partial ones (through LDS).  Time form: the threads run along the tile's
// (step, lane) elements; the peaks kernel gives a wave max(B, 64) steps at a time and reduces
// across the wave's lanes.
// Gains kernel: a tile is `g_blocks` blocks of `g_lanes` lanes with the H blocks before them, two
// copies of it in LDS (the window maximum's doubling steps go from one to the other).
struct LevelForm {
  int kind = kLevelTime;
  int K = 0, B = 0, H = 0;
  int lanes = 0;         // lanes of a tile: K (time form) or a power of two in [8, 64]
  int rows = 0;          // steps of a tile: max(B, 256), a multiple of B
  int chunk = 0;         // streams form: steps of a row group, rows / (256 / lanes); time form: max(B, 64), a wave's
  int piece = 0;         // min(chunk, B)
  int lds_bytes = 0;     // peaks kernel, streams form: 4 lanes rows / piece; time form: 0
  int lane_tiles = 0;    // ceil(K / lanes)
  int g_lanes = 0;       // lanes of a gains tile: at most `lanes`, halved until the tile fits
  int g_blocks = 0;      // blocks a gains tile forms gains for
  int g_lds_bytes = 0;   // 8 g_lanes (g_blocks + H)
  int g_lane_tiles = 0;  // ceil(K / g_lanes)
  bool ok() const { return rows > 0; }
};

// How a push falls onto the block grid and into a form's tiles.
struct LevelCut {
  int64_t outs = 0;     // steps emitted: emitted(n0 + steps) - emitted(n0)
  int64_t u_in0 = 0;    // the push's first step on the u axis: 2 B + n0 mod B
  int64_t u_in1 = 0;    // ... and the end of the push: u_in0 + steps
  int64_t e0u = 0;      // emitted(n0) on the u axis, in [B, u_in0]: the carried steps are [e0u, u_in0)
  int64_t e1u = 0;      // emitted(n0 + steps) on it, in [e0u, u_in1]: the next carry is [e1u, u_in1)
  int64_t nq = 0;       // blocks [0, nq) are complete after the push, block nq is the running one: nq >= 2
  int64_t npk = 0;      // rows of the push's peaks: nq + H, row r being block r - H
  int64_t p_tiles = 0;  // tiles of the peaks kernel: blocks [2, nq] in tiles of `rows` steps, by lane tiles
  int64_t g_tiles = 0;  // tiles of the gains kernel (0 where nothing is emitted)
  int64_t a_tiles = 0;  // tiles of the apply kernel (0 where nothing is emitted)
  int64_t a_u0 = 0;     // the first apply tile's first step: e0u rounded down to a block
  int p_grid = 0, g_grid = 0, a_grid = 0;  // workgroups (a_grid >= 1: the carry is always written)
  bool ok() const { return p_grid > 0; }
};

// 1 <= K <= 2048, B a power of two in [8, 1024], 0 <= H <= 4096
bool level_shape_ok(int K, int B, int H);
// target, gmax, floor in [2^-60, 2^60], squelch 0 or in that range (a NaN is in no range)
bool level_params_ok(float target, float gmax, float floor, float squelch);
// a stride in [K, 2^31]
bool level_stride_ok(int K, int64_t stride);

// Rule 7: max(n_r, B (floor(N / B) - 1)), the steps emitted once the count is N >= n_r.
int64_t level_emitted(uint64_t N, uint64_t n_r, int B);
// The steps a push of `steps` at count n0 emits.  0 outside 0 <= steps <= 2^31 - 1, n_r <= n0 <= 2^62.
int64_t level_steps(uint64_t n0, uint64_t n_r, int64_t steps, int B);

// !ok() outside a valid shape.
LevelForm choose_level(int K, int B, int H);

// !ok() outside 1 <= steps <= 2^31 - 1, n_r <= n0, n0 + steps <= 2^62, a form that is ok.
LevelCut level_cut(const LevelForm &f, uint64_t n0, uint64_t n_r, int64_t steps);

// Floats of one carry: (2 B - 1) K unemitted steps, K running peaks, (H + 2) K block peaks.
inline size_t level_carry_floats(int K, int B, int H) { return (size_t)(2 * B - 1 + 1 + H + 2) * (size_t)K; }

}  // namespace zfft
