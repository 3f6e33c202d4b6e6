// zfft_tap.cpp -- the channel taps of libzfft.so: digital down-converters with state on the
// plan's input samples (C-ABI and rule: zfft.h; kernel: tap_kernels.hip; form chooser, counts,
// design and table: zfft_tap_plan.h).  Nothing runs inside zfft_process*.  The
// count, the carries and the host push's staging go through the producers' shared path
// (zfft_stream.h): the sample count is the host's, so the counts and the phase words of a push are
// known when it is enqueued, and a tap opened or closed between two pushes needs no device state
// but its table row, uploaded on the plan's stream behind whatever is enqueued.
#include <algorithm>
#include <vector>

#include "zfft.h"
#include "zfft_stream.h"

using namespace zfft;

namespace zfft {

struct TapState {
  int max = 0, len = 0;        // max_taps, max_len
  int layout = 0;              // hook zfft__plan_tap_layout: 0 = the chooser's staging layout
  std::vector<TapOpen> slots;  // per slot; all zeros but `slot` while it is closed (open: T >= 1)
  std::vector<char> dirty;     // a slot's part of `pin` may still be read by an enqueued copy
  DevBuf tab;                  // a row of len entries c[k] per slot
  float2 *pin = nullptr;       // the page-locked staging of the slots' table uploads
  StreamState s;               // samples given; two carries of len - 1 samples; zfft_tap_push's staging
  ~TapState() { if (pin) (void)hipHostFree(pin); }
};

void tap_release(zfft_plan *p) {
  delete p->tap;
  p->tap = nullptr;
}

}  // namespace zfft

namespace {

constexpr StreamNames kNames{"tap", "n_samples", "sample"};

int need_on(const zfft_plan *p) { return p->tap ? ZFFT_OK : fail(ZFFT_EINVAL, "taps are off (zfft_plan_taps)"); }

int need_slot(const zfft_plan *p, int32_t slot) {
  return slot >= 0 && slot < p->tap->max ? ZFFT_OK : fail(ZFFT_EINVAL, "tap: slot out of range");
}

// The open taps in slot order.
int open_taps(const TapState *t, TapOpen *out) {
  int n = 0;
  for (const TapOpen &k : t->slots)
    if (k.T) out[n++] = k;
  return n;
}

// A checked push of n_samples >= 1 from device memory, enqueued on the caller's stream.
int push_on(zfft_plan *p, const void *d_iq, int64_t n_samples, void *d_out, void *hip_stream) {
  TapState *t = p->tap;
  if (!d_iq) return fail(ZFFT_EINVAL, "tap push: null input");
  TapOpen taps[kTapMaxTaps];
  TapItems items;
  const int ntaps = open_taps(t, taps);
  const TapForm f = choose_tap(t->s.n, n_samples, t->len, taps, ntaps, &items, t->layout);
  if (!f.ok()) return fail(ZFFT_EINTERNAL, "tap push: no form for this call");
  if (f.total > 0 && !d_out) return fail(ZFFT_EINVAL, "tap push: null output");
  hipStream_t st;
  int rc = begin_call(p, hip_stream, &st);
  if (rc) return rc;
  hipError_t e = launch_tap_push(d_iq, p->cfg.in_dtype, n_samples, t->len, f, items, t->tab.as<float2>(),
                                 t->s.carry_in(), t->s.carry_out(), (float2 *)d_out, st);
  if (e != hipSuccess) return hip_fail(e, "tap_push");
  mark(p, st, "tap_push");
  return stream_commit(p, t->s, n_samples, st);
}

}  // namespace

// Measurement hook (not part of include/zfft.h): the staging layout of the plan's pushes -- 0 the
// chooser's, else that pad shift (31: the plain array, or 3 .. 9).  The outputs do not depend on it.
extern "C" int zfft__plan_tap_layout(zfft_plan *p, int32_t shift) {
  if (!p || !p->tap || (shift && shift != kTapNoPad && (shift < kTapPadMin || shift > kTapPadMax))) return ZFFT_EINVAL;
  p->tap->layout = shift;
  return ZFFT_OK;
}

extern "C" {

int zfft_plan_taps(zfft_plan *p, int32_t max_taps, int32_t max_len) {
  int rc = enter(p);
  if (rc) return rc;
  if (max_taps == 0 && max_len == 0) {
    rc = quiesce(p);  // an enqueued push may still use all of it
    if (rc) return rc;
    tap_release(p);
    return ZFFT_OK;
  }
  if (max_taps < 1 || max_taps > kTapMaxTaps || max_len < 1 || max_len > kTapMaxLen)
    return fail(ZFFT_EINVAL, "taps: max_taps in [1, 64] and max_len in [1, 2048], or 0, 0 (off)");
  if (p->cfg.flip_input) return fail(ZFFT_EUNSUPPORTED, "taps: flip_input = 1 has no continuous time axis");
  rc = quiesce(p);
  if (rc) return rc;
  tap_release(p);
  TapState *t = p->tap = new TapState;
  t->max = max_taps, t->len = max_len;
  const size_t tab_bytes = (size_t)max_taps * max_len * sizeof(float2);
  if (t->tab.ensure(tab_bytes) != hipSuccess ||
      stream_alloc(t->s, (size_t)std::max(1, max_len - 1)) != hipSuccess ||  // (never an empty buffer)
      hipHostMalloc((void **)&t->pin, tab_bytes, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    tap_release(p);
    return fail(ZFFT_ENOMEM, "tap allocation failed");
  }
  (void)tap_conflict_model();  // the chooser's table, here and not in the first push
  for (int i = 0; i < max_taps; ++i) t->slots.push_back(TapOpen{0, 0, 0, 0, i});
  t->dirty.assign((size_t)max_taps, 0);
  return stream_restart(p, t->s, kNames, 0);
}

int zfft_tap_shape(const zfft_plan *p, int32_t *max_taps, int32_t *max_len) {
  if (!p || !max_taps || !max_len) return fail(ZFFT_EINVAL, "null argument");
  *max_taps = p->tap ? p->tap->max : 0, *max_len = p->tap ? p->tap->len : 0;
  return need_on(p);
}

int zfft_tap_open(zfft_plan *p, int32_t slot, int64_t freq_word, int32_t decim, int32_t n_taps, const float *h) {
  int rc = enter(p);
  if (!rc) rc = need_on(p);
  if (!rc) rc = need_slot(p, slot);
  if (rc) return rc;
  TapState *t = p->tap;
  if (!h || decim < 1 || decim > kTapMaxDecim || n_taps < 1 || n_taps > t->len ||
      freq_word < -((int64_t)1 << 31) || freq_word >= ((int64_t)1 << 31))
    return fail(ZFFT_EINVAL, "tap_open: freq_word in [-2^31, 2^31), decim in [1, 512], n_taps in [1, max_len], taps given");
  if (t->dirty[slot]) {  // an enqueued upload may still read this slot's staging
    // done_ev lies behind every upload: once it has passed nothing is pending, and only otherwise
    // does a second open of the slot wait on the host
    if (hipEventQuery(p->done_ev) != hipSuccess) {
      (void)hipGetLastError();  // (hipErrorNotReady is not an error of ours)
      rc = quiesce(p);
      if (rc) return rc;
    }
    std::fill(t->dirty.begin(), t->dirty.end(), 0);
  }
  float2 *stage = t->pin + (size_t)slot * t->len;
  rc = zfft_tap_table(freq_word, n_taps, h, (float *)stage);
  if (rc) return rc;
  rc = use_stream(p, p->stream);  // behind the enqueued pushes, which may still read the row
  if (rc) return rc;
  hipError_t e = hipMemcpyAsync(t->tab.as<float2>() + (size_t)slot * t->len, stage, (size_t)n_taps * sizeof(float2),
                                hipMemcpyHostToDevice, p->stream);
  if (e != hipSuccess) return hip_fail(e, "tap table upload");
  t->dirty[slot] = 1;
  t->slots[slot] = TapOpen{freq_word, decim, n_taps, t->s.n, slot};
  return done_on(p, p->stream);
}

int zfft_tap_close(zfft_plan *p, int32_t slot) {
  int rc = enter(p);
  if (!rc) rc = need_on(p);
  if (!rc) rc = need_slot(p, slot);
  if (rc) return rc;
  if (!p->tap->slots[slot].T) return fail(ZFFT_EINVAL, "tap_close: the slot is not open");
  p->tap->slots[slot] = TapOpen{0, 0, 0, 0, slot};  // (an enqueued push has its items by value)
  return ZFFT_OK;
}

int zfft_tap_info(const zfft_plan *p, int32_t slot, int32_t *is_open, int64_t *freq_word, int32_t *decim,
                  int32_t *n_taps, uint64_t *n_open, double *group_delay) {
  if (!p || !is_open || !freq_word || !decim || !n_taps || !n_open || !group_delay)
    return fail(ZFFT_EINVAL, "null argument");
  int rc = need_on(p);
  if (!rc) rc = need_slot(p, slot);
  if (rc) return rc;
  const TapOpen &k = p->tap->slots[slot];  // (zeros while it is closed)
  *is_open = k.T > 0;
  *freq_word = k.fw, *decim = k.D, *n_taps = k.T, *n_open = k.n_open;
  *group_delay = k.T ? 0.5 * (k.T - 1) : 0.0;
  return ZFFT_OK;
}

int zfft_tap_counts(const zfft_plan *p, int64_t n_samples, int64_t *counts) {
  if (!p || !counts) return fail(ZFFT_EINVAL, "null argument");
  int rc = need_on(p);
  if (rc) return rc;
  if (n_samples < 0 || n_samples > kTapMaxPush) return fail(ZFFT_EINVAL, "tap_counts: n_samples in [0, 2^31 - 1]");
  const TapState *t = p->tap;
  for (const TapOpen &k : t->slots) counts[k.slot] = k.T ? tap_count(t->s.n, k.n_open, n_samples, k.D) : 0;
  return ZFFT_OK;
}

int zfft_tap_push_device(zfft_plan *p, const void *d_iq, int64_t n_samples, void *d_out, void *hip_stream) {
  int rc = enter(p);
  if (!rc) rc = need_on(p);
  if (rc || n_samples == 0) return rc;
  rc = stream_check_push(p->tap->s, kNames, n_samples);
  return rc ? rc : push_on(p, d_iq, n_samples, d_out, hip_stream);
}

int zfft_tap_push(zfft_plan *p, const void *iq, int64_t n_samples, void *out, int64_t *counts_out) {
  int rc = enter(p);
  if (!rc) rc = need_on(p);
  if (rc) return rc;
  if (n_samples < 0 || n_samples > kTapMaxPush) return fail(ZFFT_EINVAL, "tap push: n_samples in [0, 2^31 - 1]");
  TapState *t = p->tap;
  std::vector<int64_t> counts((size_t)t->max);
  rc = zfft_tap_counts(p, n_samples, counts.data());
  if (rc) return rc;
  if (counts_out) std::copy(counts.begin(), counts.end(), counts_out);
  if (n_samples == 0) return ZFFT_OK;
  rc = stream_check_push(t->s, kNames, n_samples);
  if (rc) return rc;
  int64_t total = 0;
  for (int64_t c : counts) total += c;
  rc = stream_host_push(p, t->s, kNames, iq, (size_t)n_samples * in_elem_bytes(p->cfg.in_dtype), out,
                        (size_t)total * sizeof(float2),
                        [=](const void *d_in, void *d_out) { return push_on(p, d_in, n_samples, d_out, p->stream); });
  if (!rc) std::fill(t->dirty.begin(), t->dirty.end(), 0);  // every upload has run
  return rc;
}

int zfft_tap_state(zfft_plan *p, uint64_t *samples_seen) {
  if (!p || !samples_seen) return fail(ZFFT_EINVAL, "null argument");
  int rc = need_on(p);
  if (!rc) *samples_seen = p->tap->s.n;
  return rc;
}

int zfft_tap_reset(zfft_plan *p, int64_t n0) {
  int rc = enter(p);
  if (!rc) rc = need_on(p);
  if (!rc) rc = stream_reset(p, p->tap->s, kNames, n0);
  if (rc) return rc;
  for (TapOpen &k : p->tap->slots)  // open taps stay open, as if opened at n0
    if (k.T) k.n_open = (uint64_t)n0;
  return ZFFT_OK;
}

}  // extern "C"
