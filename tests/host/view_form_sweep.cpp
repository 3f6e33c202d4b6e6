// view_form_sweep.cpp -- stand-alone sweep of choose_view (csrc/zfft_view_plan.cpp) over its
// domain, built with ASan + UBSan by tests/test_viewport_host.py: every push gets a form inside
// its own domain -- tiles that cover the width within 256 columns (or one pixel), workgroups
// that cover every group, slices that cover a group -- with the edge limits of count, group
// length and pending rows included; outside the domain it refuses.  No HIP, no plan.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "zfft.h"
#include "zfft_view_plan.h"

using namespace zfft;

static long g_bad = 0;
static void check(bool ok, const char *what, int count, int m, int pending, int span, int width, const ViewForm &f) {
  if (ok) return;
  if (++g_bad <= 20)
    std::printf("FAIL %s: count=%d m=%d pending=%d span=%d width=%d -> kind=%d team=%d px=%d tiles=%d groups=%d "
                "k=%d s=%d slice=%d gy=%d\n",
                what, count, m, pending, span, width, f.kind, f.team, f.px, f.tiles, f.groups, f.k, f.s, f.slice_rows,
                f.gy);
}

int main() {
  const int counts[] = {1, 2, 15, 16, 37, 127, 128, 129, 7000, 65535, 65536, 69632, 1 << 20, 1 << 30};
  const int ms[] = {1, 2, 5, 15, 16, 17, 64, 127, 128, 129, 3000, 65535, 65536};
  const int spans[] = {1, 2, 63, 64, 65, 256, 257, 512, 1000, 8192, 65535, 65536};
  long n = 0;
  int seen[3][5] = {};
  for (int count : counts)
    for (int m : ms)
      for (int span : spans)
        for (int width : {1, 2, 3, 7, 32, 63, 64, 255, 256, 257, 1920, 65536}) {
          if (width > span) continue;
          for (int pending : {0, 1, m / 2, m - 1}) {
            if (pending >= m) continue;
            const ViewForm f = choose_view(count, m, pending, span, width);
            ++n;
            check(f.ok(), "a form for every push", count, m, pending, span, width, f);
            if (!f.ok()) continue;
            const int bmax = (span + width - 1) / width;
            const int64_t groups = ((int64_t)pending + count + m - 1) / m;
            check(f.groups == groups, "the groups the push touches", count, m, pending, span, width, f);
            check(f.px >= 1 && (f.px == 1 || f.px * bmax <= kViewTileCols), "a tile within 256 columns", count, m,
                  pending, span, width, f);
            check((int64_t)f.px * f.tiles >= width && (int64_t)f.px * (f.tiles - 1) < width && f.tiles <= 65535,
                  "tiles cover the width", count, m, pending, span, width, f);
            check(f.gy >= 1 && (int64_t)f.gy * f.tiles <= (int64_t)1 << 31, "a launchable grid", count, m, pending, span,
                  width, f);
            if (f.kind == kViewLines) {
              check(f.s == 1 && f.k >= 1 && (int64_t)f.gy * f.k >= groups && (int64_t)(f.gy - 1) * f.k < groups,
                    "workgroups cover the groups", count, m, pending, span, width, f);
              check(f.team == (m >= 16 ? 4 : 1) && (f.team == 4 || f.k % 4 == 0), "the team of the group length", count,
                    m, pending, span, width, f);
            } else {
              check(f.kind == kViewSplit && f.team == kViewWaves && f.k == 1 && f.s >= 2, "split: one group a slice",
                    count, m, pending, span, width, f);
              check((int64_t)f.s * f.slice_rows >= m && (int64_t)(f.s - 1) * f.slice_rows < m && f.slice_rows >= 32,
                    "slices cover the group", count, m, pending, span, width, f);
              check(f.gy == f.groups * f.s && groups * f.tiles < 512, "split only below a full grid", count, m, pending,
                    span, width, f);
            }
            if (f.kind >= 0 && f.kind < 3 && f.team >= 0 && f.team < 5) seen[f.kind][f.team] = 1;
          }
        }
  check(seen[kViewLines][4] && seen[kViewLines][1] && seen[kViewSplit][4], "every form is returned somewhere", 0, 0, 0,
        0, 0, ViewForm());
  const int bad[][5] = {{0, 1, 0, 8, 8},  {-1, 1, 0, 8, 8}, {1, 0, 0, 8, 8},     {1, 65537, 0, 8, 8}, {1, 5, 5, 8, 8},
                        {1, 5, -1, 8, 8}, {1, 1, 0, 8, 9},  {1, 1, 0, 8, 0},     {1, 1, 0, 65537, 8}, {1, 1, 0, 0, 0},
                        {INT32_MAX, INT32_MAX, 0, 8, 8},    {1, 1, 0, INT32_MAX, INT32_MAX}};
  for (const auto &b : bad)
    check(!choose_view(b[0], b[1], b[2], b[3], b[4]).ok(), "refused", b[0], b[1], b[2], b[3], b[4], ViewForm());
  // the bucket edges: monotone, exact ends, sizes within one of each other
  for (int span : spans)
    for (int width : {1, 7, 64, 1920, 65536}) {
      if (width > span) continue;
      int64_t lo = INT64_MAX, hi = 0, prev = zfft_viewport_edge(3, 3 + span, width, 0);
      bool ok = prev == 3 && zfft_viewport_edge(3, 3 + span, width, width) == 3 + span;
      for (int x = 1; x <= width; ++x) {
        const int64_t e = zfft_viewport_edge(3, 3 + span, width, x);
        lo = e - prev < lo ? e - prev : lo;
        hi = e - prev > hi ? e - prev : hi;
        prev = e;
      }
      check(ok && lo >= 1 && hi - lo <= 1, "bucket edges", 0, 0, 0, span, width, ViewForm());
    }
  check(zfft_viewport_edge(0, 8, 9, 0) == -1 && zfft_viewport_edge(0, 8, 4, 5) == -1 &&
            zfft_viewport_edge(INT32_MAX - 1, INT32_MAX, 1, 1) == INT32_MAX,
        "edge limits", 0, 0, 0, 0, 0, ViewForm());
  if (g_bad) {
    std::printf("view_form_sweep: %ld checks failed over %ld keys\n", g_bad, n);
    return 1;
  }
  std::printf("view_form_sweep: ok (%ld keys)\n", n);
  return 0;
}
