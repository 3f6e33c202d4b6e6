// zfft_welch.cpp -- the Welch half of a call: the window tables and one runner per form
// (zfft_welch_plan.h); run_welch launches what choose_welch names.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "zfft.h"
#include "zfft_median_bias.h"
#include "zfft_plan.h"
#include "zfft_welch_plan.h"

namespace zfft {
namespace {

// In-place radix-2 DFT (forward, exp(-2 pi i k n / N)), N a power of two, float64.
void fft64(std::vector<double> &re, std::vector<double> &im) {
  const size_t n = re.size();
  for (size_t i = 1, j = 0; i < n; ++i) {
    size_t bit = n >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j |= bit;
    if (i < j) std::swap(re[i], re[j]), std::swap(im[i], im[j]);
  }
  for (size_t len = 2; len <= n; len <<= 1) {
    const double a = -2.0 * M_PI / (double)len;
    for (size_t i = 0; i < n; i += len)
      for (size_t k = 0; k < len / 2; ++k) {
        const double c = std::cos(a * (double)k), sn = std::sin(a * (double)k);
        const size_t u = i + k, v = u + len / 2;
        const double tr = re[v] * c - im[v] * sn, ti = re[v] * sn + im[v] * c;
        re[v] = re[u] - tr, im[v] = im[u] - ti;
        re[u] += tr, im[u] += ti;
      }
  }
}

// welch builds get_window(window, nperseg); nperseg = min(N, L_d) (short-input branch).
int ensure_window(zfft_plan *p, int nperseg) {
  if (p->win_len == nperseg) return ZFFT_OK;
  int rc = quiesce(p);
  if (rc) return rc;
  std::vector<double> w;
  if (p->cfg.window_kind == ZFFT_WIN_ARRAY) {
    if (nperseg != p->cfg.n_fft)
      return fail(ZFFT_EINVAL, "window is longer than input signal (array window of length "
                               "n_fft, decimated frame shorter than n_fft)");
    w.assign(p->user_window.begin(), p->user_window.end());
  } else if (!make_window(p->cfg.window_kind, p->cfg.window_param, nperseg, w)) {
    return fail(ZFFT_EINVAL, "window generation failed");
  }
  std::vector<float> wf(nperseg);
  double ss = 0.0;
  for (int i = 0; i < nperseg; ++i) {
    wf[i] = (float)w[i];
    ss += w[i] * w[i];
  }
  hipError_t e = p->win.ensure(p->cfg.n_fft * sizeof(float));
  if (e != hipSuccess) return fail(ZFFT_ENOMEM, "window allocation failed");
  e = hipMemcpy(p->win.p, wf.data(), nperseg * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) return hip_fail(e, "window upload");
  if (nperseg == p->cfg.n_fft && p->cfg.n_fft >= kWelch4Min) {  // (four-step capable sizes)
    // the four-step Welch subtracts the segment mean after its transform: X = FFT(x w) -
    // mean FFT(w) (scipy's detrend='constant' is linear); FFT(w) of the float32 window, fp64
    std::vector<double> re(wf.begin(), wf.end()), im(nperseg, 0.0);
    fft64(re, im);
    std::vector<float2> wft(nperseg);
    for (int k = 0; k < nperseg; ++k) wft[k] = make_float2((float)re[k], (float)im[k]);
    e = p->winf.ensure(nperseg * sizeof(float2));
    if (e == hipSuccess) e = hipMemcpy(p->winf.p, wft.data(), nperseg * sizeof(float2), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(e, "window transform upload");
  }
  p->win_len = nperseg;
  p->win_ss = ss;
  return ZFFT_OK;
}

// Density scaling 1 / (fs sum(w^2)) with the mean over `div` segments folded in (csd average='mean').
float density_scale(const zfft_plan *p, int div) { return (float)(1.0 / (p->cfg.fs * p->win_ss * (double)div)); }

// One workgroup per frame (Stockham or in-place DIF), nf frames from x: dB rows, partial sums and
// their second launch, fused mean lines, or every segment's bins -- whatever pl.out names.
int welch_onewg(zfft_plan *p, const WelchPlan &pl, WelchGeom w, const float2 *x, int64_t Ld, float *out, int nf,
                hipStream_t st) {
  w.split = p->last_split = nf == pl.chunk ? pl.split : pl.split_last;
  WelchLines ln;
  if (pl.out == WelchOut::FusedLines) {
    ln.grp = pl.grp;
    ln.lines = pl.lines;
    ln.scale_tail = density_scale(p, pl.tail);
  }
  if (pl.out == WelchOut::Parts) {
    if (p->wparts.ensure(pl.wparts) != hipSuccess) return fail(ZFFT_ENOMEM, "Welch workspace allocation failed");
    w.parts = p->wparts.as<float>();
  }
  const hipError_t e = launch_welch_rows(x, Ld, p->win.as<float>(), p->tw.as<float2>(), w, out, nf, st,
                                         pl.out == WelchOut::Segs, ln);
  return e == hipSuccess ? ZFFT_OK : hip_fail(e, "welch_rows launch");
}

// Four-step, nf frames from x in one launch set: the intermediate Z goes through HBM between the
// column and the row pass (chunks that keep it in the Infinity Cache measured slower).
int welch_four(zfft_plan *p, const WelchPlan &pl, WelchGeom w, const float2 *x, int64_t Ld, float *out, int nf,
               hipStream_t st) {
  w.fused_mean = pl.fused_mean;
  hipError_t e = p->means.ensure(pl.means);
  if (e == hipSuccess) e = p->z4.ensure(pl.z4);
  if (e != hipSuccess) return fail(ZFFT_ENOMEM, "four-step Welch workspace allocation failed");
  e = launch_welch4(x, Ld, p->win.as<float>(), p->tw.as<float2>(), p->tws.as<float2>(),
                    w.fused_mean ? p->winf.as<float2>() : nullptr, w, p->means.as<float2>(), p->z4.as<float2>(),
                    out, nf, st, pl.out == WelchOut::Segs);
  return e == hipSuccess ? ZFFT_OK : hip_fail(e, "welch4 launch");
}

// The segment scratch route: per chunk of frames every segment's bins, then welch_select's
// detector per frame or per line of pl.grp segments (mean lines: their mean).
int welch_segs(zfft_plan *p, const WelchPlan &pl, const WelchGeom &w, const float2 *x, int64_t Ld, int frames,
               float *d_rows, hipStream_t st) {
  if (p->wsegs.ensure(pl.wsegs) != hipSuccess) return fail(ZFFT_ENOMEM, "Welch segment workspace allocation failed");
  // over n segments: the median's bias, the mean's 1 / n
  auto inv = [&](int n) {
    return p->average == ZFFT_AVG_MEDIAN ? (float)(1.0 / median_bias(n))
           : p->average == ZFFT_AVG_MEAN ? (float)(1.0 / (double)n) : 1.f;
  };
  WelchSelect sel{pl.nseg, p->cfg.n_win, row_length(p), p->average, inv(pl.sel_div)};
  if (pl.grp) {  // per line: its own segment count (grp, or the tail's)
    sel.grp = pl.grp;
    sel.lines = pl.lines;
    sel.inv_bias_tail = inv(pl.tail);
  }
  const bool four = pl.fft == WelchFft::FourStep;
  for (int f0 = 0; f0 < frames; f0 += pl.chunk) {
    const int nf = std::min(pl.chunk, frames - f0);
    const int rc = (four ? welch_four : welch_onewg)(p, pl, w, x + (int64_t)f0 * Ld, Ld, p->wsegs.as<float>(), nf, st);
    if (rc) return rc;
    mark(p, st, four ? "welch4_segs" : "welch_segs");
    const hipError_t e = launch_welch_select(p->wsegs.as<float>(), sel, pl.sel,
                                             d_rows + (int64_t)f0 * pl.lines * p->cfg.n_win, nf, st);
    if (e != hipSuccess) return hip_fail(e, "welch_select launch");
    mark(p, st, pl.sel == WelchSel::MeanLines ? "welch_lines" : "welch_select");
  }
  return ZFFT_OK;
}

}  // namespace

int run_welch(zfft_plan *p, const float2 *x, int64_t Ld, int frames, float *d_rows, hipStream_t st) {
  const WelchPlan pl = choose_welch({p->cfg.n_fft, p->cfg.n_win, Ld, frames, p->welch, p->average,
                                     p->seg_per_line, p->lines_route, p->avg_cap});
  if (pl.rc) return fail(pl.rc, pl.why);
  int rc = ensure_window(p, pl.nperseg);  // (also sets win_ss, which the scales need)
  if (rc) return rc;
  const int N = p->cfg.n_fft;
  WelchGeom w;
  w.n_fft = N;
  w.log2n = 0;
  while ((1 << w.log2n) < N) ++w.log2n;
  w.n_win = p->cfg.n_win;
  w.nperseg = pl.nperseg;
  w.step = pl.step;
  w.nseg = pl.nseg;
  w.scale = density_scale(p, pl.scale_div);
  if (onesided(p)) {
    w.onesided = 1;
    w.row_a = N / 2 - p->cfg.n_win / 2;
    w.row_len = row_length(p);
  }
  if (pl.out == WelchOut::Segs) return welch_segs(p, pl, w, x, Ld, frames, d_rows, st);
  const bool four = pl.fft == WelchFft::FourStep;
  rc = (four ? welch_four : welch_onewg)(p, pl, w, x, Ld, d_rows, frames, st);
  if (rc) return rc;
  mark(p, st, pl.out == WelchOut::FusedLines ? "welch_lines" : four ? "welch4" : "welch_rows");
  return ZFFT_OK;
}

}  // namespace zfft
