// zfft_welch_plan.h -- which Welch form a call takes, as a value: a pure host function of the
// plan's settings, the decimated frame length and the frames per call.  No HIP, no plan:
// zfft_welch.cpp launches what it returns, the launchers in zfft_kernels.hip guard its
// invariants and tests/test_welch_plan.py pins it without a device.
#pragma once

#include <cstddef>
#include <cstdint>

namespace zfft {

// --- domains of the kernel forms (zfft_kernels.hip ties its template switches to them) ---
constexpr int kMaxLdsFft = 16384;  // one workgroup per frame holds at most this many points in LDS
constexpr int kWelch4Min = 4096;   // four-step: N = N1 * 256 with N1 >= 16
// the in-place DIF kernel covers 1024 <= N <= 16384 (N = 16384: one 1024-thread frame per
// workgroup, 139 KB of LDS, a 4-value prefetch to stay within 128 VGPRs)
#ifndef ZFFT_DIF_MAX
#define ZFFT_DIF_MAX 16384
#endif
constexpr int kDifMin = 1024, kDifMax = ZFFT_DIF_MAX;
#ifndef ZFFT_WELCH_ONEWG_MAX
#define ZFFT_WELCH_ONEWG_MAX 16384
#endif
constexpr int kWelchOneWgMax = ZFFT_WELCH_ONEWG_MAX;  // auto: one workgroup per frame up to here
static_assert(kDifMax <= kMaxLdsFft && kWelchOneWgMax <= kMaxLdsFft, "one-workgroup forms end at kMaxLdsFft");
// welch_select holds a column's keys in registers up to kSelRegSegs segments, in LDS (median
// only) up to kSelLdsSegs (256 B per segment and wave: 64 KB at most), else re-reads the scratch
constexpr int kSelRegSegs = 32, kSelLdsSegs = 256;
// Segment scratch of the median / max detectors per chunk of frames.  A cap of the Infinity
// Cache's size (256 MB, so that welch_select reads what the Welch kernels just wrote) measured
// slower than one launch set wherever it splits a call (cfg1's 4096 frames, 532 MB: 2.95 against
// 2.61 ms), so the cap only bounds the workspace.
#ifndef ZFFT_AVG_SCRATCH_MB
#define ZFFT_AVG_SCRATCH_MB 1024
#endif
constexpr size_t kAvgScratchBytes = (size_t)ZFFT_AVG_SCRATCH_MB << 20;

// A frame's Welch segments (scipy.signal.welch: nperseg = min(N, L_d), the short-input branch;
// noverlap = nperseg // 2) and its lines (zfft_plan_segments_per_line = g): the only place that
// computes them.
struct WelchSegments {
  int64_t nperseg, step, nseg;
  int64_t grp;    // segments per line, 1 <= g < nseg; 0: the whole frame is one row
  int64_t lines;  // rows per frame: ceil(nseg / grp), or 1
  int64_t tail;   // segments of the last line (grp 0: nseg)
};
WelchSegments welch_segments(int64_t Ld, int n_fft, int g);  // Ld >= 1, n_fft >= 2, g >= 0

// In-place DIF Welch for few frames per call: each frame's units (segments, or with by_lines
// whole lines) over `split` workgroups, enough to fill the chip (about 768 workgroups at
// N = 4096); at least 2 segments or 1 line per part, from 4 segments or 2 lines; 1 for full
// batches and outside the DIF kernel's domain.  The kernel gives part y the units
// [y per, (y + 1) per), per = ceil(units / split): every part starts inside its frame,
// (split - 1) per < units.
int welch_split(int n_fft, int64_t units, int frames, bool by_lines);

struct WelchKey {
  int n_fft, n_win;
  int64_t Ld;        // decimated frame length
  int frames;        // frames per call
  int welch;         // zfft_plan_welch: 0 auto, 1 one workgroup per frame, 2 four-step
  int average;       // zfft_plan_average: ZFFT_AVG_MEAN / _MEDIAN / _MAX
  int seg_per_line;  // zfft_plan_segments_per_line
  int lines_route;   // hook zfft__plan_lines_route: 1 = mean lines through the scratch too
  size_t cap_bytes;  // segment scratch cap (hook zfft__plan_average_cap); 0: kAvgScratchBytes
};

enum class WelchFft { Stockham, Dif, FourStep };
// What the Welch launch of a frame writes: its dB row; (Dif, split > 1) linear partial sums that
// a second launch adds; its mean lines; or every segment's bins into the scratch for welch_select.
enum class WelchOut { Row, Parts, FusedLines, Segs };
// How welch_select holds a column's keys (Segs only); MeanLines: the mean of each line instead.
enum class WelchSel { None, Reg4, Reg8, Reg16, Reg24, Reg32, Lds, Scratch, MeanLines };

struct WelchPlan {
  int rc;           // ZFFT_OK, or zfft_plan_welch's refusal of the mode at this n_fft
  const char *why;  // rc != ZFFT_OK: the error message (a string literal), else nullptr
  int nperseg, step, nseg, grp, lines, tail;  // welch_segments
  WelchFft fft;
  WelchOut out;
  int split, split_last;  // welch_split of a whole chunk and of the call's last (shorter) chunk
  int fused_mean;         // four-step: segment means from the column pass (nperseg == n_fft)
  // Integer divisors of the scale factors (the runner folds them into 1 / (fs sum(w^2) div) or
  // the detector's bias): of the Welch kernels' scale -- nseg, grp (fused lines) or 1 (Segs) --
  // and of welch_select's -- grp, else nseg; `tail` divides both forms' last line
  int scale_div, sel_div;
  int64_t out_floats;  // floats per frame the Welch launch writes
  int chunk;           // frames per launch set (Segs: what fits the scratch cap, at least 1)
  WelchSel sel;
  size_t wparts, wsegs, means, z4;  // workspace bytes
};

// rc / message of a Welch mode at n_fft (zfft_plan_welch refuses with them).
int welch_mode_rc(int n_fft, int mode, const char **why);
WelchPlan choose_welch(const WelchKey &k);
const char *welch_fft_name(WelchFft f);  // "stockham", "dif", "four"
const char *welch_out_name(WelchOut o);  // "row", "parts", "lines", "segs"
const char *welch_sel_name(WelchSel s);  // "none", "reg4", ..., "lds", "scratch", "mean_lines"

}  // namespace zfft
