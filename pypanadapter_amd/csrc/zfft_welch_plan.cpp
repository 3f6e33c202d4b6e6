// zfft_welch_plan.cpp -- the Welch form chooser (zfft_welch_plan.h): the transform, what it
// writes, the split, the chunks and the selection form of a call, in one pure function.
#include "zfft_welch_plan.h"

#include <algorithm>

#include "zfft.h"

namespace zfft {

WelchSegments welch_segments(int64_t Ld, int n_fft, int g) {
  WelchSegments s;
  s.nperseg = Ld < n_fft ? Ld : n_fft;
  s.step = s.nperseg - s.nperseg / 2;
  s.nseg = (Ld - s.nperseg) / s.step + 1;
  s.grp = g >= 1 && g < s.nseg ? g : 0;
  s.lines = s.grp ? (s.nseg + s.grp - 1) / s.grp : 1;
  s.tail = s.nseg - (s.lines - 1) * s.grp;
  return s;
}

int welch_split(int n_fft, int64_t units, int frames, bool by_lines) {
  if (n_fft < kDifMin || n_fft > kDifMax || units < (by_lines ? 2 : 4)) return 1;
  const int fpb = n_fft / 16 >= 256 ? 1 : 256 / (n_fft / 16);  // frames per workgroup
  const int64_t blocks = ((int64_t)frames + fpb - 1) / fpb;
  const int target = 768 * 256 / std::max(256, n_fft / 16);  // workgroups that fill the chip
  if (blocks >= target / 2) return 1;
  const int64_t want = std::min<int64_t>((target + blocks - 1) / blocks, by_lines ? units : units / 2);
  const int64_t per = (units + want - 1) / want;
  return (int)((units + per - 1) / per);  // every part non-empty
}

int welch_mode_rc(int n_fft, int mode, const char **why) {
  *why = nullptr;
  if (mode < 0 || mode > 2) {
    *why = "welch mode must be 0 (auto), 1 (one workgroup) or 2 (four-step)";
    return ZFFT_EINVAL;
  }
  if (mode == 1 && n_fft > kMaxLdsFft) {
    *why = "one-workgroup Welch holds at most 16384 points in LDS";
    return ZFFT_EUNSUPPORTED;
  }
  if (mode == 2 && n_fft < kWelch4Min) {
    *why = "four-step Welch needs n_fft >= 4096 (N1 = n_fft/256 >= 16)";
    return ZFFT_EINVAL;
  }
  return ZFFT_OK;
}

// The smallest register form that holds the keys; beyond kSelRegSegs the median's bisection
// keeps them in LDS while they fit, and max (one pass) reads the scratch.
static WelchSel sel_form(int keys, bool median) {
  if (keys <= 4) return WelchSel::Reg4;
  if (keys <= 8) return WelchSel::Reg8;
  if (keys <= 16) return WelchSel::Reg16;
  if (keys <= 24) return WelchSel::Reg24;
  if (keys <= kSelRegSegs) return WelchSel::Reg32;
  return median && keys <= kSelLdsSegs ? WelchSel::Lds : WelchSel::Scratch;
}

WelchPlan choose_welch(const WelchKey &k) {
  WelchPlan w{};
  w.rc = welch_mode_rc(k.n_fft, k.welch, &w.why);
  if (w.rc != ZFFT_OK) return w;
  const int N = k.n_fft;
  const WelchSegments s = welch_segments(k.Ld, N, k.seg_per_line);
  w.nperseg = (int)s.nperseg, w.step = (int)s.step, w.nseg = (int)s.nseg;
  w.grp = (int)s.grp, w.lines = (int)s.lines, w.tail = (int)s.tail;
  const bool mean = k.average == ZFFT_AVG_MEAN;
  // auto: four-step above 16384 (the only form there); N <= 16384 runs one workgroup per
  // frame, the in-place DIF kernel where it covers N and the segments are whole
  const bool four = k.welch == 2 || (k.welch == 0 && N > kWelchOneWgMax);
  const bool dif = !four && w.nperseg == N && N >= kDifMin && N <= kDifMax;
  w.fft = four ? WelchFft::FourStep : dif ? WelchFft::Dif : WelchFft::Stockham;
  // mean lines from the in-place DIF kernel are fused (its LINES variant writes each line from
  // the segment loop: faster than the scratch route at every g measured); the
  // median and max detectors take the segments' densities one by one, and lines from the
  // Stockham kernel (its fused form measured slower) or the four-step form are reduced per
  // group: both through the segment scratch
  const bool fused = w.grp > 0 && mean && dif && k.lines_route != 1;
  const bool segs = (!mean || w.grp > 0) && !fused;
  w.scale_div = segs ? 1 : fused ? w.grp : w.nseg;
  w.sel_div = w.grp ? w.grp : w.nseg;
  w.out_floats = (int64_t)(segs ? w.nseg : w.lines) * k.n_win;
  w.chunk = k.frames;
  if (segs) {
    // the frames in chunks whose segment scratch stays within the cap; at least one frame
    const size_t per = (size_t)w.out_floats * sizeof(float);
    const size_t cap = k.cap_bytes ? k.cap_bytes : kAvgScratchBytes;
    w.chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)k.frames, cap / per));
    w.wsegs = (size_t)w.chunk * per;
    // keys per column: the frame's segments, or those of a full line
    w.sel = w.grp && mean ? WelchSel::MeanLines : sel_form(w.sel_div, k.average == ZFFT_AVG_MEDIAN);
  }
  // few frames per launch (the reference's one): each frame's segments or lines over several workgroups
  w.split = w.split_last = 1;
  if (dif) {
    const int64_t units = fused ? w.lines : w.nseg;
    const int last = k.frames % w.chunk;
    w.split = welch_split(N, units, w.chunk, fused);
    w.split_last = last ? welch_split(N, units, last, fused) : w.split;
  }
  w.out = fused ? WelchOut::FusedLines : segs ? WelchOut::Segs : w.split > 1 ? WelchOut::Parts : WelchOut::Row;
  if (w.out == WelchOut::Parts) w.wparts = (size_t)k.frames * w.split * k.n_win * sizeof(float);
  if (four) {
    w.fused_mean = w.nperseg == N ? 1 : 0;
    // per frame of a launch set: the column pass's partial sums per segment (256-column groups
    // of 16) and the intermediate Z (nseg x N complex64)
    w.means = (size_t)w.chunk * w.nseg * std::max(1, N / 256 / 16) * 8;
    w.z4 = (size_t)w.chunk * w.nseg * N * 8;
  }
  return w;
}

const char *welch_fft_name(WelchFft f) {
  return f == WelchFft::FourStep ? "four" : f == WelchFft::Dif ? "dif" : "stockham";
}
const char *welch_out_name(WelchOut o) {
  return o == WelchOut::Row ? "row" : o == WelchOut::Parts ? "parts" : o == WelchOut::FusedLines ? "lines" : "segs";
}
const char *welch_sel_name(WelchSel s) {
  static const char *const names[] = {"none", "reg4", "reg8", "reg16", "reg24", "reg32", "lds", "scratch", "mean_lines"};
  return names[(int)s];
}

}  // namespace zfft
