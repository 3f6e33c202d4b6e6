// history_form_sweep.cpp -- stand-alone sweep of choose_history and of the row history's quantiser
// (csrc/zfft_history_plan.cpp) over their domains, built with ASan + UBSan by
// tests/test_history_host.py: every window gets a form inside its own domain -- tiles that cover
// the width within a wave's columns after the unaligned head (or one pixel), workgroups that
// cover every line, slices that cover a group -- and outside the domain the chooser refuses; the
// quantiser is idempotent over every code, monotone, and within 0.513 step inside the range.
// No HIP, no plan.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "zfft.h"
#include "zfft_history_plan.h"

using namespace zfft;

static long g_bad = 0;
static void check(bool ok, const char *what, int lines, int m, int span, int width, int format, const HistForm &f) {
  if (ok) return;
  if (++g_bad <= 20)
    std::printf("FAIL %s: lines=%d m=%d span=%d width=%d format=%d -> kind=%d px=%d tiles=%d k=%d s=%d slice=%d gy=%d\n",
                what, lines, m, span, width, format, f.kind, f.px, f.tiles, f.k, f.s, f.slice_rows, f.gy);
}

int main() {
  const int lines_[] = {1, 2, 3, 7, 511, 512, 1080, 8191, 8192};
  const int ms[] = {1, 2, 5, 15, 16, 17, 64, 127, 128, 129, 3000, 65535, 65536};
  const int spans[] = {1, 2, 15, 16, 17, 63, 64, 65, 253, 256, 257, 1009, 1024, 1025, 8192, 65535, 65536};
  long n = 0;
  int seen[3] = {};
  for (int format = 0; format < 3; ++format)
    for (int lines : lines_)
      for (int m : ms)
        for (int span : spans)
          for (int width : {1, 2, 3, 7, 32, 63, 64, 255, 256, 257, 1009, 1920, 4096, 65536}) {
            if (width > span || (int64_t)lines * width > ((int64_t)1 << 25)) continue;
            const HistForm f = choose_history(lines, m, span, width, format);
            ++n;
            check(f.ok(), "a form for every window", lines, m, span, width, format, f);
            if (!f.ok()) continue;
            const int bmax = (span + width - 1) / width;
            const int room = hist_tile_cols(format) - (hist_lane_cols(format) - 1);
            check(f.lines == lines, "the window's lines", lines, m, span, width, format, f);
            check(f.px >= 1 && (f.px == 1 || f.px * bmax <= room), "a tile within a wave's columns", lines, m, span,
                  width, format, f);
            check((int64_t)f.px * f.tiles >= width && (int64_t)f.px * (f.tiles - 1) < width && f.tiles <= 65535,
                  "tiles cover the width", lines, m, span, width, format, f);
            check(f.gy >= 1 && (int64_t)f.gy * f.tiles <= (int64_t)1 << 31, "a launchable grid", lines, m, span, width,
                  format, f);
            if (f.kind == kHistWhole) {
              check(f.s == 1 && f.k >= 1 && (int64_t)f.gy * f.k >= lines && (int64_t)(f.gy - 1) * f.k < lines,
                    "workgroups cover the lines", lines, m, span, width, format, f);
            } else {
              check(f.kind == kHistSliced && f.k == 1 && f.s >= 2, "sliced: one line a slice", lines, m, span, width,
                    format, f);
              check((int64_t)f.s * f.slice_rows >= m && (int64_t)(f.s - 1) * f.slice_rows < m && f.slice_rows >= 32,
                    "slices cover the group", lines, m, span, width, format, f);
              check(f.gy == lines * f.s && (int64_t)lines * f.tiles < 512, "sliced only below a full grid", lines, m,
                    span, width, format, f);
            }
            if (f.kind >= 0 && f.kind < 3) seen[f.kind] = 1;
          }
  check(seen[kHistWhole] && seen[kHistSliced], "every form is returned somewhere", 0, 0, 0, 0, 0, HistForm());
  const int bad[][5] = {{0, 1, 8, 8, 2},     {-1, 1, 8, 8, 2},        {8193, 1, 8, 8, 2}, {1, 0, 8, 8, 2},
                        {1, 65537, 8, 8, 2}, {1, 1, 8, 9, 2},         {1, 1, 8, 0, 2},    {1, 1, 65537, 8, 2},
                        {1, 1, 8, 8, 3},     {1, 1, 8, 8, -1},        {8192, 1, 8192, 4097, 2},
                        {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX, 0}};
  for (const auto &b : bad)
    check(!choose_history(b[0], b[1], b[2], b[3], b[4]).ok(), "refused", b[0], b[1], b[2], b[3], b[4], HistForm());
  check(hist_stride(1) == 16 && hist_stride(16) == 16 && hist_stride(17) == 32 && hist_stride(151) == 160 &&
            hist_stride(65536) == 65536,
        "stored stride", 0, 0, 0, 0, 0, HistForm());

  // ---- the quantiser
  const double ranges[][2] = {{-220, -20}, {-160, -40}, {-250.5, -99.25}, {0, 100}, {-1e-3, 1e-3}, {-300, 300}};
  long q_bad = 0;
  for (int format : {kHistU16, kHistU8})
    for (const auto &r : ranges) {
      HistQuant q;
      if (!hist_quant(format, r[0], r[1], &q)) {
        ++q_bad;
        continue;
      }
      float prev = -INFINITY;
      for (int c = 1; c <= q.K + 1; ++c) {  // idempotent over every code, values ascending
        const float v = hist_value(q, (uint16_t)c);
        if (hist_code(q, v) != c || !(v >= prev)) ++q_bad;
        prev = v;
      }
      if (!std::isnan(hist_value(q, 0)) || hist_code(q, NAN) != 0 || hist_code(q, -INFINITY) != 1 ||
          hist_code(q, INFINITY) != q.K + 1 || hist_code(q, (float)r[0]) != 1 || hist_code(q, (float)r[1]) != q.K + 1)
        ++q_bad;
      const int steps = 200001;
      const double a = r[0] - 0.05 * (r[1] - r[0]), b = r[1] + 0.05 * (r[1] - r[0]);
      int last = 0;
      std::vector<float> vs(steps);
      for (int i = 0; i < steps; ++i) vs[i] = (float)(a + (b - a) * i / (steps - 1));
      for (int i = 0; i < steps; ++i) {  // monotone, and 0.513 step inside the range
        const int c = hist_code(q, vs[i]);
        if (c < last) ++q_bad;
        last = c;
        if (vs[i] >= (float)r[0] && vs[i] <= (float)r[1] &&
            std::fabs((double)hist_value(q, (uint16_t)c) - (double)vs[i]) > 0.513 * (double)q.step)
          ++q_bad;
      }
    }
  HistQuant q;
  if (hist_quant(3, -1, 1, &q) || hist_quant(kHistU8, 1, 1, &q) || hist_quant(kHistU8, 2, 1, &q) ||
      hist_quant(kHistU16, NAN, 1, &q) || hist_quant(kHistU8, -INFINITY, 1, &q) || hist_quant(kHistU8, 0, INFINITY, &q) ||
      !hist_quant(kHistF32, NAN, NAN, &q))
    ++q_bad;
  uint16_t codes[4];
  const float v4[4] = {-150.f, -100.f, NAN, 1e30f};
  float back[4];
  if (zfft_history_codes(kHistU8, -150, -50, v4, 4, codes) != ZFFT_OK || codes[0] != 1 || codes[1] != 128 ||
      codes[2] != 0 || codes[3] != 255 || zfft_history_values(kHistU8, -150, -50, codes, 4, back) != ZFFT_OK ||
      back[0] != -150.f || !std::isnan(back[2]) || back[3] != -50.f ||
      zfft_history_codes(kHistF32, -150, -50, v4, 4, codes) != ZFFT_EINVAL ||
      zfft_history_codes(kHistU8, -50, -150, v4, 4, codes) != ZFFT_EINVAL)
    ++q_bad;
  codes[0] = 256;
  if (zfft_history_values(kHistU8, -150, -50, codes, 1, back) != ZFFT_EINVAL) ++q_bad;
  if (g_bad || q_bad) {
    std::printf("history_form_sweep: %ld form checks and %ld quantiser checks failed over %ld keys\n", g_bad, q_bad, n);
    return 1;
  }
  std::printf("history_form_sweep: ok (%ld keys)\n", n);
  return 0;
}
