// zfft_tap_plan.cpp -- the pure host side of the channel taps (zfft_tap_plan.h): choose_tap, the
// output counts, the Kaiser design and the modulated table.  No HIP: built into libzfft.so and,
// stand-alone under ASan + UBSan, into tests/host/tap_form_sweep.cpp (which supplies set_error
// and the window it links against).
#include "zfft_tap_plan.h"

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <string>
#include <vector>

namespace zfft {

void set_error(const std::string &msg);  // zfft_plan.cpp

namespace {

int tap_fail(const char *msg) {
  set_error(msg);
  return ZFFT_EINVAL;
}

}  // namespace

int tap_conflict(int D, int shift) {
  int sum = 0;
  for (int k = 0; k < 16; ++k)
    for (int base : {0, 5, 17, 31}) {
      // the lanes' slots ascend strictly, so all addresses differ: the degree is the fullest bank
      int banks[32] = {}, worst = 1;
      for (int l = 0; l < 32; ++l) worst = std::max(worst, ++banks[tap_slot(kTapMaxLen + base + l * D - k, shift) & 31]);
      sum += worst;
    }
  return sum;
}

const int *tap_conflict_model() {
  static const std::vector<int> model = [] {
    std::vector<int> m((size_t)(kTapMaxDecim + 1) * kTapLayouts);
    for (int D = 1; D <= kTapMaxDecim; ++D)
      for (int c = 0; c < kTapLayouts; ++c) m[(size_t)D * kTapLayouts + c] = tap_conflict(D, kTapLayoutShifts[c]);
    return m;
  }();
  return model.data();
}

TapForm choose_tap(uint64_t n0, int64_t n, int max_len, const TapOpen *taps, int ntaps, TapItems *items, int layout) {
  TapForm f;
  if (layout && layout != kTapNoPad && (layout < kTapPadMin || layout > kTapPadMax)) return f;
  if (n < 1 || n > kTapMaxPush || n0 > kTapMaxCount || max_len < 1 || max_len > kTapMaxLen || ntaps < 0 ||
      ntaps > kTapMaxTaps || (ntaps && (!taps || !items)))
    return f;
  int halo = 0;
  for (int i = 0; i < ntaps; ++i) {
    const TapOpen &t = taps[i];
    if (t.D < 1 || t.D > kTapMaxDecim || t.T < 1 || t.T > max_len || t.n_open > n0 || t.fw < -((int64_t)1 << 31) ||
        t.fw >= ((int64_t)1 << 31))
      return f;
    halo = std::max(halo, t.T - 1);
  }
  int S = kTapSpanMax;
  while (S > kTapSpanMin && (n + S - 1) / S < kTapSpansWanted) S /= 2;
  const int64_t spans = (n + S - 1) / S, H = max_len - 1;
  f.halo = halo;
  const int *model = tap_conflict_model();  // (built by zfft_plan_taps: nothing to compute in a push)
  double best = -1.0;
  for (int c = 0; c < kTapLayouts; ++c) {  // (the plain array first: it wins a tie)
    double cost = 0.0;
    for (int i = 0; i < ntaps; ++i) cost += (double)taps[i].T / taps[i].D * model[(size_t)taps[i].D * kTapLayouts + c];
    if (best < 0.0 || cost < best) best = cost, f.pad_shift = kTapLayoutShifts[c];
  }
  if (layout) f.pad_shift = layout;
  f.lds_bytes = (tap_slot(halo + S - 1, f.pad_shift) + 1) * 8;
  if (f.lds_bytes > kTapLdsMax) return f;
  // no tap open: the carry's part only (at least the last span: a launch is never empty)
  f.first_span = ntaps ? 0 : (int)std::min(spans - 1, std::max<int64_t>(0, n - H) / S);
  f.grid = (int)(spans - f.first_span);
  f.ntaps = ntaps;
  int64_t off = 0;
  for (int i = 0; i < ntaps; ++i) {
    const TapOpen &t = taps[i];
    TapItem &it = items->t[i];
    it.r0 = (int64_t)stream_first(n0, t.D);
    const uint64_t first = n0 + (uint64_t)it.r0;  // m D of the first output: n_open <= n0
    it.count = (int32_t)tap_count(n0, t.n_open, n, t.D);
    it.out_off = off;
    // the phase words wrap at 2^32 exactly: unsigned 32-bit products of the low words
    it.ph0 = (uint32_t)t.fw * (uint32_t)first;
    it.dph = (uint32_t)t.fw * (uint32_t)t.D;
    it.D = t.D, it.T = t.T, it.slot = t.slot;
    off += it.count;
  }
  f.total = off;
  f.span = S;
  return f;
}

// The design's formula for any length (zfft_tap_design, zfft_resamp_design): arguments checked by the caller.
int kaiser_sinc(int T, double cutoff, double beta, double *h_out) {
  // the symmetric Kaiser of T points: the periodic one of T - 1 (zfft_window_values) and its
  // first value again; T <= 2 is a constant window, which the normalisation removes
  std::vector<double> w((size_t)T, 1.0);
  if (T >= 3) {
    if (zfft_window_values(ZFFT_WIN_KAISER, &beta, T - 1, w.data()) != ZFFT_OK) return ZFFT_EINVAL;
    w[T - 1] = w[0];
  }
  const double fc = 2.0 * cutoff, alpha = 0.5 * (T - 1);  // scipy's firwin: the band edge in Nyquist units
  double sum = 0.0;
  for (int k = 0; k < T; ++k) {
    const double m = (double)k - alpha, x = M_PI * fc * m;
    const double sinc = x == 0.0 ? 1.0 : std::sin(x) / x;
    h_out[k] = fc * sinc * w[k];
    sum += h_out[k];
  }
  for (int k = 0; k < T; ++k) h_out[k] /= sum;  // unit gain at DC
  return ZFFT_OK;
}

}  // namespace zfft

using namespace zfft;

// Test hooks (not part of include/zfft.h; no plan, no device): tap_count, and the form and items
// of a push -- form8 = {span, halo, lds_bytes, first_span, grid, ntaps, total, pad_shift}; per tap
// items6 = {r0, out_off, ph0, dph, count, slot}.
extern "C" int64_t zfft__tap_count(uint64_t n0, uint64_t n_open, int64_t n, int32_t D) {
  return tap_count(n0, n_open, n, D);
}
extern "C" int zfft__tap_conflict(int32_t D, int32_t shift) {
  return D >= 1 && D <= kTapMaxDecim && shift >= kTapPadMin && shift <= kTapNoPad ? tap_conflict(D, shift) : -1;
}
extern "C" int zfft__tap_form(uint64_t n0, int64_t n, int32_t max_len, int32_t ntaps, const int64_t *fw,
                              const int32_t *D, const int32_t *T, const uint64_t *n_open, int64_t *form8,
                              int64_t *items6) {
  if (ntaps < 0 || ntaps > kTapMaxTaps || !form8 || (ntaps && (!fw || !D || !T || !n_open || !items6))) return -1;
  TapOpen taps[kTapMaxTaps];
  TapItems items;
  for (int i = 0; i < ntaps; ++i) taps[i] = TapOpen{fw[i], D[i], T[i], n_open[i], i};
  const TapForm f = choose_tap(n0, n, max_len, taps, ntaps, &items);
  if (!f.ok()) return -1;
  const int64_t v[8] = {f.span, f.halo, f.lds_bytes, f.first_span, f.grid, f.ntaps, f.total, f.pad_shift};
  std::copy(v, v + 8, form8);
  for (int i = 0; i < ntaps; ++i) {
    const TapItem &t = items.t[i];
    const int64_t w[6] = {t.r0, t.out_off, (int64_t)t.ph0, (int64_t)t.dph, t.count, t.slot};
    std::copy(w, w + 6, items6 + 6 * i);
  }
  return 0;
}

extern "C" {

int zfft_tap_design(int32_t n_taps, double cutoff, double beta, double *h_out) {
  if (!h_out || n_taps < 1 || n_taps > kTapMaxLen || !(cutoff > 0.0 && cutoff < 0.5) || !(beta >= 0.0) ||
      !std::isfinite(beta))
    return tap_fail("tap_design: n_taps in [1, 2048], 0 < cutoff < 0.5 cycles per sample, beta >= 0");
  return kaiser_sinc(n_taps, cutoff, beta, h_out);
}

int zfft_tap_table(int64_t freq_word, int32_t n_taps, const float *h, float *c_out) {
  if (!h || !c_out || n_taps < 1 || n_taps > kTapMaxLen || freq_word < -((int64_t)1 << 31) ||
      freq_word >= ((int64_t)1 << 31))
    return tap_fail("tap_table: n_taps in [1, 2048], freq_word in [-2^31, 2^31)");
  for (int k = 0; k < n_taps; ++k) {
    const uint32_t w = (uint32_t)freq_word * (uint32_t)k;  // (fw k) mod 2^32
    const double a = 2.0 * M_PI * ((double)w / 4294967296.0);
    c_out[2 * k] = (float)((double)h[k] * std::cos(a));
    c_out[2 * k + 1] = (float)((double)h[k] * std::sin(a));
  }
  return ZFFT_OK;
}

}  // extern "C"
