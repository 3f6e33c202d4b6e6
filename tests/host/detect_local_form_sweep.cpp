// detect_local_form_sweep.cpp -- stand-alone sweep of choose_detect_local
// (csrc/zfft_detect_plan.cpp) over its domain, built with ASan + UBSan by
// tests/test_detect_local_host.py: for every row_len in [1, 65536] x half_window in {1, 16, 32, 33, 64, 65, 128}
// x guard in {0, 128} the tiles cover every column exactly once, the tile and its halos stay
// inside the LDS budget, the mask words of a window's side hold the half window, the passes
// stay inside the scratch and the grid inside the tiles; outside the domain it refuses.  No HIP,
// no plan.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "zfft_detect_plan.h"

using namespace zfft;

static long g_bad = 0;
static void check(bool ok, const char *what, int row_len, int count, int h, int gd, const DetectLocalForm &f) {
  if (ok) return;
  if (++g_bad <= 20)
    std::printf("FAIL %s: row_len=%d count=%d h=%d guard=%d -> tile=%d tiles=%d halo=%d words=%d grid=%d chunk=%d\n",
                what, row_len, count, h, gd, f.tile, f.tiles, f.halo, f.words, f.grid, f.chunk_rows);
}

int main() {
  constexpr int kMaxCells = 768;  // 256 + 2 * 256: the cells the kernel file's bit planes hold
  const int counts[] = {1, 3, 300, 69632, 1 << 26};
  long n = 0;
  for (int row_len = 1; row_len <= kDetectMaxCols; ++row_len)
    for (int h : {1, 16, 32, 33, 64, 65, 128})
      for (int gd : {0, 128})
        for (int count : counts) {
          const int n_win = row_len + (row_len & 1);
          const DetectLocalForm f = choose_detect_local(row_len, n_win, count, h, gd);
          ++n;
          check(f.ok(), "a form for every width", row_len, count, h, gd, f);
          if (!f.ok()) continue;
          check(f.tile == kDetectLocalTile && f.tile % 64 == 0 && f.tile <= 1024, "a tile of whole waves", row_len,
                count, h, gd, f);
          // tile i is [i * tile, min(row_len, (i + 1) * tile)): disjoint by construction; they
          // cover [0, row_len) when the last one starts inside the row and ends at or past it
          check((int64_t)f.tiles * f.tile >= row_len && (int64_t)(f.tiles - 1) * f.tile < row_len && f.tiles >= 1,
                "the tiles cover every column once", row_len, count, h, gd, f);
          check(f.halo == h + gd, "the halo reaches the farthest reference cell", row_len, count, h, gd, f);
          check(f.lds_keys() == f.tile + 2 * f.halo && f.lds_keys() <= kMaxCells,
                "tile and halos inside the LDS planes", row_len, count, h, gd, f);
          check((f.words == 1 || f.words == 2 || f.words == 4) && h <= 32 * f.words && (f.words == 1 || h > 16 * f.words),
                "the fewest mask words that hold the half window", row_len, count, h, gd, f);
          check(f.chunk_rows >= 1 && f.chunk_rows <= count &&
                    (size_t)f.chunk_rows * n_win * sizeof(float) <= kDetectLocalScratch,
                "a pass inside the scratch", row_len, count, h, gd, f);
          check(f.chunk_rows == count || (size_t)(f.chunk_rows + 1) * n_win * sizeof(float) > kDetectLocalScratch,
                "the largest such pass", row_len, count, h, gd, f);
          check(f.grid >= 1 && f.grid <= kDetectLocalGridMax && (int64_t)f.grid <= (int64_t)f.chunk_rows * f.tiles,
                "grid within the tiles", row_len, count, h, gd, f);
        }
  const DetectLocalForm none;
  for (int row_len : {0, -1, kDetectMaxCols + 1, INT32_MIN, INT32_MAX})
    check(!choose_detect_local(row_len, kDetectMaxCols, 1, 16, 2).ok(), "refused width", row_len, 1, 16, 2, none);
  check(!choose_detect_local(64, 63, 1, 16, 2).ok(), "refused stride", 64, 1, 16, 2, none);
  for (int count : {0, -1, INT32_MIN}) check(!choose_detect_local(512, 512, count, 16, 2).ok(), "refused count", 512, count, 16, 2, none);
  for (int h : {0, -1, 129, INT32_MAX}) check(!choose_detect_local(512, 512, 1, h, 0).ok(), "refused half window", 512, 1, h, 0, none);
  for (int gd : {-1, 129, INT32_MIN}) check(!choose_detect_local(512, 512, 1, 16, gd).ok(), "refused guard", 512, 1, 16, gd, none);
  check(!choose_detect_local(512, 512, 1, 16, 2, 2047).ok(), "refused scratch below a row", 512, 1, 16, 2, none);
  check(choose_detect_local(512, 512, 300, 16, 2, 2048 * 7 + 5).chunk_rows == 7, "a small scratch sets the pass", 512, 300,
        16, 2, none);
  if (g_bad) {
    std::printf("detect_local_form_sweep: %ld checks failed over %ld keys\n", g_bad, n);
    return 1;
  }
  std::printf("detect_local_form_sweep: ok (%ld keys)\n", n);
  return 0;
}
