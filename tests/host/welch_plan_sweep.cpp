// welch_plan_sweep.cpp -- stand-alone sweep of choose_welch (csrc/zfft_welch_plan.cpp) over its
// domain, built with ASan + UBSan by tests/test_welch_plan.py: the invariants the Welch kernels'
// safety rests on hold for whatever the chooser returns, and its byte counts and products do
// not overflow (UBSan would stop the program).  No HIP, no plan.  for_each_key is the key set;
// a program that compares the chooser against another one includes this file with
// WELCH_PLAN_SWEEP_NO_MAIN defined and walks the same keys.
#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "zfft.h"
#include "zfft_welch_plan.h"

using namespace zfft;

// Keys whose decimated frames exceed the card's memory are skipped: allocation refuses them first.
static const int64_t kCardBytes = (int64_t)288 * 1000 * 1000 * 1000;

template <class Fn>
static void for_each_key(Fn fn) {
  const int Fs[] = {1, 2, 5, 47, 48, 383, 384, 767, 768, 4096, 65535};
  for (int N = 32; N <= 65536; N *= 2) {
    const int64_t step = N - N / 2;
    // short input, nseg 1 .. 4 (around the split floor), the selection thresholds, long frames
    const int64_t Lds[] = {1, 2, N - 1, N, N + step - 1, N + step, N + 2 * step, N + 3 * step, N + 4 * step,
                           N + 16 * step, N + 31 * step, N + 32 * step, N + 255 * step, N + 256 * step,
                           N + 400 * step, ((int64_t)1 << 20) + 7, (int64_t)1 << 30};
    for (int W : {2, N - 1, N / 8, N / 8 + 1, N})
      for (int64_t Ld : Lds)
        for (int frames : Fs) {
          if ((int64_t)frames * Ld * 8 > kCardBytes) continue;
          const int64_t nseg = welch_segments(Ld, N, 0).nseg;
          const int64_t per = nseg * W * 4;  // one frame's segment scratch
          const int64_t gs[] = {0, 1, 4, 5, 8, 9, 16, 17, 24, 25, 32, 33, 256, 257, nseg - 1, nseg, nseg + 1};
          for (int welch = 0; welch <= 2; ++welch)
            for (int average : {ZFFT_AVG_MEAN, ZFFT_AVG_MEDIAN, ZFFT_AVG_MAX})
              for (int route = 0; route <= 1; ++route)
                for (int64_t g : gs) {
                  if (g < 0 || g > INT_MAX) continue;
                  for (int64_t cap : {(int64_t)0, per - 1, per * 5 / 2})
                    fn(WelchKey{N, W, Ld, frames, welch, average, (int)g, route, (size_t)cap});
                }
        }
  }
}

#ifndef WELCH_PLAN_SWEEP_NO_MAIN
static long g_bad = 0;
static void check(bool ok, const char *what, const WelchKey &k, const WelchPlan &w) {
  if (ok) return;
  if (++g_bad <= 20)
    std::printf("FAIL %s: N=%d W=%d Ld=%lld frames=%d welch=%d avg=%d g=%d route=%d cap=%zu -> %s %s split=%d/%d "
                "lines=%d chunk=%d %s\n", what, k.n_fft, k.n_win, (long long)k.Ld, k.frames, k.welch, k.average,
                k.seg_per_line, k.lines_route, k.cap_bytes, welch_fft_name(w.fft), welch_out_name(w.out), w.split,
                w.split_last, w.lines, w.chunk, welch_sel_name(w.sel));
}

// part y of `split` takes the units [y per, (y + 1) per), per = ceil(units / split): none empty
static bool parts_ok(int64_t units, int split) {
  if (split < 1 || split > units) return false;
  const int64_t per = (units + split - 1) / split;
  return (split - 1) * per < units;
}

int main() {
  long n = 0, refused = 0;
  for_each_key([&](const WelchKey &k) {
    const WelchPlan w = choose_welch(k);
    ++n;
    const int N = k.n_fft;
    const bool bad_mode = (k.welch == 1 && N > 16384) || (k.welch == 2 && N < 4096);
    check((w.rc != ZFFT_OK) == bad_mode && (w.rc == ZFFT_OK) == (w.why == nullptr), "refusal", k, w);
    if (w.rc != ZFFT_OK) {
      ++refused;
      return;
    }
    const bool four = w.fft == WelchFft::FourStep, dif = w.fft == WelchFft::Dif;
    const bool fused = w.out == WelchOut::FusedLines, segs = w.out == WelchOut::Segs;
    const bool mean = k.average == ZFFT_AVG_MEAN;
    // segments and lines
    const WelchSegments s = welch_segments(k.Ld, N, k.seg_per_line);
    check(w.nperseg == s.nperseg && w.step == s.step && w.nseg == s.nseg && w.grp == s.grp && w.lines == s.lines &&
              w.tail == s.tail, "welch_segments", k, w);
    check(w.nseg >= 1 && (int64_t)(w.nseg - 1) * w.step + w.nperseg <= k.Ld, "segments inside the frame", k, w);
    check(w.grp == 0 ? (w.lines == 1 && w.tail == w.nseg)
                     : (w.grp < w.nseg && w.lines == (w.nseg + w.grp - 1) / w.grp && w.tail >= 1 && w.tail <= w.grp &&
                        (int64_t)(w.lines - 1) * w.grp + w.tail == w.nseg), "lines", k, w);
    // (zfft_line_count is welch_segments(...).lines behind its argument checks)
    check(w.lines == (k.seg_per_line == 0 || k.Ld < N ? 1
                      : k.seg_per_line >= w.nseg      ? 1 : (w.nseg + k.seg_per_line - 1) / k.seg_per_line),
          "lines == zfft_line_count", k, w);
    // transform domains
    check(!four || N >= 4096, "FourStep only for N >= 4096", k, w);
    check(four || N <= 16384, "one-workgroup forms only for N <= 16384", k, w);
    check(!dif || (N >= kDifMin && N <= kDifMax && w.nperseg == N), "Dif inside its domain, whole segments", k, w);
    check(four == (k.welch == 2 || (k.welch == 0 && N > kWelchOneWgMax)), "forced mode is honoured", k, w);
    // outputs
    check(!fused || (dif && mean && w.grp >= 1 && k.lines_route == 0), "FusedLines: Dif, mean, grp >= 1", k, w);
    check(w.out != WelchOut::Parts || (dif && mean && w.grp == 0 && w.split > 1 && w.lines == 1),
          "Parts: a split Dif row", k, w);
    check(w.out != WelchOut::Row || (mean && w.grp == 0 && w.split == 1), "Row: one unsplit mean row", k, w);
    check(segs == ((!mean || w.grp > 0) && !fused), "Segs: detectors and unfused lines", k, w);
    // split: every part non-empty, whole chunks and the last one
    const int64_t units = fused ? w.lines : w.nseg;
    check(parts_ok(units, w.split) && parts_ok(units, w.split_last), "every split part is non-empty", k, w);
    check(dif || (w.split == 1 && w.split_last == 1), "split only in the Dif kernel", k, w);
    check(segs || w.split == w.split_last, "one launch set unless chunked", k, w);
    // chunks and workspaces
    const unsigned __int128 per = (unsigned __int128)w.out_floats * 4;
    check(w.out_floats == (int64_t)(segs ? w.nseg : w.lines) * k.n_win, "floats per frame", k, w);
    check(w.chunk >= 1 && w.chunk <= k.frames && (segs || w.chunk == k.frames), "1 <= chunk <= frames", k, w);
    if (segs) {
      const size_t cap = k.cap_bytes ? k.cap_bytes : kAvgScratchBytes;
      check(w.chunk == 1 || per * w.chunk <= cap, "chunk within the cap", k, w);
      check(w.chunk == k.frames || per * (w.chunk + 1) > cap, "chunk as large as the cap allows", k, w);
    }
    check(w.wsegs == (segs ? per * w.chunk : 0), "wsegs bytes", k, w);
    check(w.wparts == (w.out == WelchOut::Parts ? (unsigned __int128)k.frames * w.split * k.n_win * 4 : 0),
          "wparts bytes", k, w);
    check(w.z4 == (four ? (unsigned __int128)w.chunk * w.nseg * N * 8 : 0) && (w.means != 0) == four &&
              w.means <= w.z4, "four-step workspaces", k, w);
    check(w.fused_mean == (four && w.nperseg == N), "fused_mean", k, w);
    check((unsigned __int128)k.frames * w.out_floats * 4 < ((unsigned __int128)1 << 63) &&
              (int64_t)w.split * k.frames <= INT_MAX, "products fit", k, w);
    // scale divisors
    check(w.scale_div == (segs ? 1 : fused ? w.grp : w.nseg) && w.sel_div == (w.grp ? w.grp : w.nseg), "divisors", k, w);
    // selection form against its key count and mode
    const int keys = w.sel_div;
    const int ns = w.sel == WelchSel::Reg4 ? 4 : w.sel == WelchSel::Reg8 ? 8 : w.sel == WelchSel::Reg16 ? 16
                   : w.sel == WelchSel::Reg24 ? 24 : w.sel == WelchSel::Reg32 ? 32 : 0;
    check((w.sel == WelchSel::None) == !segs, "a selection exactly with Segs", k, w);
    check((w.sel == WelchSel::MeanLines) == (segs && mean), "MeanLines: mean lines from the scratch", k, w);
    const int below = ns <= 8 ? ns - 4 : ns - 8;  // the next smaller form's slots (4, 8, 16, 24, 32)
    check(!ns || (keys <= ns && keys > below && ns <= kSelRegSegs), "smallest register form", k, w);
    check(w.sel != WelchSel::Lds || (k.average == ZFFT_AVG_MEDIAN && keys > kSelRegSegs && keys <= kSelLdsSegs),
          "Lds: median, 32 < keys <= 256", k, w);
    check(w.sel != WelchSel::Scratch || (keys > kSelRegSegs && (k.average == ZFFT_AVG_MAX || keys > kSelLdsSegs)),
          "Scratch: beyond the registers (max) or the LDS (median)", k, w);
  });
  if (g_bad) {
    std::printf("welch_plan_sweep: %ld checks failed over %ld keys\n", g_bad, n);
    return 1;
  }
  std::printf("welch_plan_sweep: ok (%ld keys, %ld refused)\n", n, refused);
  return 0;
}
#endif
