// zfft_view_plan.h -- which form of the display viewport's reduction (view_kernels.hip; rule in
// zfft.h) a push takes, as a value: a pure host function of the push's rows, the group length,
// the pending rows and the geometry.  No HIP, no plan: zfft_viewport.cpp launches what it
// returns, the launcher guards its invariants and tests/test_viewport_host.py sweeps it without
// a device.
#pragma once

#include <cstdint>

namespace zfft {

constexpr int kViewMaxHeight = 8192;
constexpr int kViewMaxPixels = 1 << 25;   // height * width
constexpr int kViewMaxGroup = 65536;      // rows_per_line
constexpr int kViewTileCols = 256;        // row columns a workgroup holds per row: 4 x 64 lanes
constexpr int kViewWaves = 4;             // waves per workgroup

enum ViewKind { kViewNone = 0, kViewLines = 1, kViewSplit = 2 };

// A push of `count` rows continues a group that holds `pending` rows (pending < m) and so touches
// groups = ceil((pending + count) / m) groups, group 0 the pending one.  A workgroup owns one
// column tile: px consecutive pixels, whose buckets together hold at most kViewTileCols columns
// (px = 1 when one bucket alone is wider: its columns then fold onto the 256 accumulators).
//   kViewLines  workgroup y reduces the whole groups [y k, (y + 1) k) one after another: `team`
//               = 4, a group's rows dealt to the four waves and combined in LDS (m >= 16), or
//               `team` = 1, one wave per group and four groups at a time (short groups).  Lines
//               complete within the push go straight to the ring; s = 1.
//   kViewSplit  too few groups to fill the chip: each group's m rows are cut into s > 1 slices of
//               slice_rows, one workgroup per (group, slice) writing a partial to the plan's
//               scratch; the finishing launch combines them.  k = 1, team = 4.
struct ViewForm {
  int kind = kViewNone;
  int team = 0;
  int px = 0, tiles = 0;        // pixels per tile, column tiles: grid.y
  int groups = 0;               // groups the push touches
  int k = 0;                    // groups per workgroup (lines)
  int s = 0, slice_rows = 0;    // slices per group and their rows (split)
  int gy = 0;                   // workgroups per tile: grid.x
  bool ok() const { return kind != kViewNone; }
};

// !ok() outside count >= 1, 1 <= m <= 65536, 0 <= pending < m, 1 <= width <= span <= 65536.
ViewForm choose_view(int count, int m, int pending, int span, int width);

}  // namespace zfft
