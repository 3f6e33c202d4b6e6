// zfft_detect_plan.h -- which form of the row detector (detect_kernels.hip; rule in zfft.h) a
// call takes, as a value: a pure host function of the row length and the rows per call.  No
// HIP, no plan: zfft_detect.cpp launches what it returns, the launcher guards its invariants
// and tests/test_detect_host.py sweeps it without a device.
#pragma once

#include <cstddef>
#include <cstdint>

namespace zfft {

constexpr int kDetectMaxCols = 65536;  // n_win's upper bound
constexpr int kDetectMaxPerRow = 32;   // K, records per row
constexpr int kDetectWord = 64;        // columns per on-flag word: one wave's ballot

// One workgroup of `waves` waves holds a row in registers, `per` keys per lane: word
// wd = i * waves + wave (i < per) is the columns [64 wd, 64 wd + 64), lane l its column
// 64 wd + l, so a load is one coalesced 256-B line per wave and a ballot is a word.  A row has
// a wave boundary every 64 columns and a per-lane chunk boundary every 64 * waves.
struct DetectForm {
  int waves = 0, per = 0;
  int grid = 0;  // workgroups: each takes the rows blockIdx.x, blockIdx.x + grid, ...
  int cols() const { return kDetectWord * waves * per; }  // the form's domain: row_len <= cols()
  bool ok() const { return waves > 0; }
};

// The narrowest form whose domain holds row_len: one wave per row up to 512 columns (the UI's
// and cfg2's rows: no LDS traffic and no barrier in the selection), 4 waves up to 2048, 16
// waves (one 1024-thread workgroup) up to 65536.  The grid is one workgroup per row up to one
// resident round of the chip.  !ok() outside 1 <= row_len <= 65536 or count < 1.
DetectForm choose_detect(int row_len, int count);

// ---- the local floor (zfft_plan_detect_local; detect_local_kernels.hip) ----
constexpr int kDetectLocalMaxHalf = 128;   // half_window's upper bound
constexpr int kDetectLocalMaxGuard = 128;  // guard's upper bound
constexpr int kDetectLocalTile = 256;      // columns (= threads) of a workgroup's tile
constexpr int kDetectLocalGridMax = 1 << 16;  // workgroups of a launch: each walks the tiles t, t + grid, ...
constexpr size_t kDetectLocalScratch = (size_t)256 << 20;  // bytes of the plan's floors scratch, at most

// One workgroup of `tile` threads takes `tile` consecutive columns of one row, a thread a column:
// it holds the tile and `halo` = guard + half_window columns on either side in LDS as
// bit-sliced keys (the columns outside the row as the pad key), `lds_keys()` cells of them.  A row has `tiles` tiles,
// tile i the columns [i * tile, min(row_len, (i + 1) * tile)), and a call count * tiles of them;
// `chunk_rows` rows go through the scratch at a time.
struct DetectLocalForm {
  int tile = 0, tiles = 0, halo = 0;
  int words = 0;       // 32-bit mask words per side of a thread's window: 1, 2 or 4 (half_window <= 32 words)
  int grid = 0;        // workgroups of a launch on min(count, chunk_rows) rows
  int chunk_rows = 0;  // rows per pass: chunk_rows * n_win floats fit `scratch_bytes`
  int lds_keys() const { return tile + 2 * halo; }
  bool ok() const { return tile > 0; }
};

// The one tile width (256: a 512-wide row is two workgroups, a 65,536-wide one 256, so one wide
// row spreads over the chip; the halo of at most 2 * 256 keys costs at most 2x the loads).
// A side of the window is 1 mask word up to half_window 32, 2 up to 64, 4 up to 128.
// !ok() outside 1 <= row_len <= n_win <= 65536, 1 <= half_window <= 128, 0 <= guard <= 128,
// count >= 1 or scratch_bytes < one row (0 = kDetectLocalScratch).
DetectLocalForm choose_detect_local(int row_len, int n_win, int count, int half_window, int guard,
                                    size_t scratch_bytes = 0);

}  // namespace zfft
