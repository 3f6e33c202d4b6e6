// zfft_view_plan.cpp -- choose_view (zfft_view_plan.h) and the viewport's bucket edge: pure host
// code, built into libzfft.so.
#include "zfft_view_plan.h"

#include <algorithm>
#include <cstddef>

#include "zfft.h"

namespace zfft {

namespace {
constexpr int kLinesGrid = 2048;   // workgroups of a large push: 8 of 4 waves on each of 256 CUs
constexpr int kSplitBelow = 512;   // fewer (group, tile) pairs than this: split the groups
constexpr int kSplitGrid = 1024;   // workgroups a split aims for (the finish walks s parts a pixel)
constexpr int kSplitMinRows = 32;  // rows per slice at least
constexpr int kTeamRows = 16;      // groups of fewer rows take one wave each
}  // namespace

ViewForm choose_view(int count, int m, int pending, int span, int width) {
  ViewForm f;
  if (count < 1 || m < 1 || m > kViewMaxGroup || pending < 0 || pending >= m || width < 1 || width > span ||
      span > 65536)
    return f;
  const int bmax = (span + width - 1) / width;
  f.px = bmax <= kViewTileCols ? std::min(width, kViewTileCols / bmax) : 1;
  f.tiles = (width + f.px - 1) / f.px;
  const int64_t groups = ((int64_t)pending + count + m - 1) / m;
  f.groups = (int)groups;
  if (groups * f.tiles < kSplitBelow && m >= 4 * kSplitMinRows) {
    const int want = std::max<int64_t>(2, kSplitGrid / (groups * f.tiles));
    const int s0 = std::min(want, m / kSplitMinRows);
    f.slice_rows = (m + s0 - 1) / s0;
    f.s = (m + f.slice_rows - 1) / f.slice_rows;  // (no empty last slice)
    if (f.s >= 2) {
      f.kind = kViewSplit;
      f.team = kViewWaves;
      f.k = 1;
      f.gy = f.groups * f.s;
      return f;
    }
  }
  f.kind = kViewLines;
  f.team = m >= kTeamRows ? kViewWaves : 1;
  f.s = 1;
  f.slice_rows = m;
  const int64_t ymax = std::max(1, kLinesGrid / f.tiles);
  int64_t k = (groups + ymax - 1) / ymax;
  if (f.team == 1) k = (k + kViewWaves - 1) / kViewWaves * kViewWaves;  // four groups at a time
  f.k = (int)k;
  f.gy = (int)((groups + k - 1) / k);
  return f;
}

}  // namespace zfft

extern "C" int64_t zfft_viewport_edge(int32_t col0, int32_t col1, int32_t width, int32_t x) {
  if (col0 < 0 || col1 <= col0 || width < 1 || width > col1 - col0 || x < 0 || x > width) return -1;
  return (int64_t)col0 + (int64_t)x * (col1 - col0) / width;
}

// Test hook (not part of include/zfft.h): the form of a push, out[0..8] = kind, team, px, tiles,
// groups, k, s, slice_rows, gy; -1 where the chooser refuses.
extern "C" int zfft__view_form(int32_t count, int32_t m, int32_t pending, int32_t span, int32_t width,
                               int32_t *out) {
  const zfft::ViewForm f = zfft::choose_view(count, m, pending, span, width);
  if (!f.ok() || !out) return -1;
  const int v[9] = {f.kind, f.team, f.px, f.tiles, f.groups, f.k, f.s, f.slice_rows, f.gy};
  for (int i = 0; i < 9; ++i) out[i] = v[i];
  return 0;
}
