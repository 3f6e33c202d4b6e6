// zfft_tap.cpp -- the channel taps of libzfft.so: digital down-converters with state on the
// plan's input samples (C-ABI and rule: zfft.h; kernel: tap_kernels.hip; form chooser, counts,
// design and table: zfft_tap_plan.h).  The model is zfft_track.cpp's: nothing
// runs inside zfft_process*.  The sample count is the host's -- every n_samples is a host
// argument and pushes are in call order -- so the counts and the phase words of a push are known
// when it is enqueued, and a tap opened or closed between two pushes needs no device state but
// its table row, uploaded on the plan's stream behind whatever is enqueued.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "zfft.h"
#include "zfft_plan.h"

using namespace zfft;

namespace {

int need_on(const zfft_plan *p) { return p->tp_max ? ZFFT_OK : fail(ZFFT_EINVAL, "taps are off (zfft_plan_taps)"); }

int need_slot(const zfft_plan *p, int32_t slot) {
  return slot >= 0 && slot < p->tp_max ? ZFFT_OK : fail(ZFFT_EINVAL, "tap: slot out of range");
}

size_t carry_len(const zfft_plan *p) { return (size_t)std::max(1, p->tp_len - 1); }  // (never an empty buffer)
float2 *carry(const zfft_plan *p, int par) { return p->tp_carry.as<float2>() + (size_t)par * carry_len(p); }

// The open taps in slot order.
int open_taps(const zfft_plan *p, TapOpen *out) {
  int n = 0;
  for (int s = 0; s < p->tp_max; ++s) {
    const zfft_plan::TapSlot &t = p->tp_slots[s];
    if (t.open) out[n++] = TapOpen{t.fw, t.D, t.T, t.n_open, s};
  }
  return n;
}

int check_push(const zfft_plan *p, int64_t n) {
  if (n < 1 || n > kTapMaxPush) return fail(ZFFT_EINVAL, "tap push: n_samples in [0, 2^31 - 1]");
  if (p->tp_n + (uint64_t)n > kTapMaxCount) return fail(ZFFT_EINVAL, "tap push: the sample count would pass 2^62");
  return ZFFT_OK;
}

// The count back to n0 and the carry to zeros, in stream order on the plan's stream.  Open taps
// stay open, as if opened at n0.
int restart(zfft_plan *p, uint64_t n0) {
  int rc = use_stream(p, p->stream);
  if (rc) return rc;
  hipError_t e = hipMemsetAsync(p->tp_carry.p, 0, 2 * carry_len(p) * sizeof(float2), p->stream);
  if (e != hipSuccess) return hip_fail(e, "tap reset");
  p->tp_n = n0;
  p->tp_par = 0;
  for (auto &t : p->tp_slots) t.n_open = n0;
  return done_on(p, p->stream);
}

}  // namespace

namespace zfft {

void tap_release(zfft_plan *p) {
  p->tp_tab.release();
  p->tp_carry.release();
  p->tp_stage.release();
  if (p->tp_pin) (void)hipHostFree(p->tp_pin);
  p->tp_pin = nullptr;
  p->tp_slots.clear();
  p->tp_dirty.clear();
  p->tp_max = p->tp_len = p->tp_par = 0;
  p->tp_layout = 0;
  p->tp_n = 0;
}

}  // namespace zfft

// Measurement hook (not part of include/zfft.h): the staging layout of the plan's pushes -- 0 the
// chooser's, else that pad shift (31: the plain array, or 3 .. 9).  The outputs do not depend on it.
extern "C" int zfft__plan_tap_layout(zfft_plan *p, int32_t shift) {
  if (!p || (shift && shift != kTapNoPad && (shift < kTapPadMin || shift > kTapPadMax))) return ZFFT_EINVAL;
  p->tp_layout = shift;
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
  if (p->cfg.flip_input)
    return fail(ZFFT_EUNSUPPORTED, "taps: flip_input = 1 has no continuous time axis");
  rc = quiesce(p);
  if (rc) return rc;
  tap_release(p);
  p->tp_max = max_taps, p->tp_len = max_len;
  const size_t tab_bytes = (size_t)max_taps * max_len * sizeof(float2);
  if (p->tp_tab.ensure(tab_bytes) != hipSuccess || p->tp_carry.ensure(2 * carry_len(p) * sizeof(float2)) != hipSuccess ||
      hipHostMalloc((void **)&p->tp_pin, tab_bytes, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    tap_release(p);
    return fail(ZFFT_ENOMEM, "tap allocation failed");
  }
  (void)tap_conflict_model();  // the chooser's table, here and not in the first push
  p->tp_slots.assign((size_t)max_taps, zfft_plan::TapSlot());
  p->tp_dirty.assign((size_t)max_taps, 0);
  return restart(p, 0);
}

int zfft_tap_shape(const zfft_plan *p, int32_t *max_taps, int32_t *max_len) {
  if (!p || !max_taps || !max_len) return fail(ZFFT_EINVAL, "null argument");
  *max_taps = p->tp_max, *max_len = p->tp_len;
  return need_on(p);
}

int zfft_tap_open(zfft_plan *p, int32_t slot, int64_t freq_word, int32_t decim, int32_t n_taps, const float *h) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (!rc) rc = need_slot(p, slot);
  if (rc) return rc;
  if (!h || decim < 1 || decim > kTapMaxDecim || n_taps < 1 || n_taps > p->tp_len ||
      freq_word < -((int64_t)1 << 31) || freq_word >= ((int64_t)1 << 31))
    return fail(ZFFT_EINVAL, "tap_open: freq_word in [-2^31, 2^31), decim in [1, 512], n_taps in [1, max_len], taps given");
  if (p->tp_dirty[slot]) {  // an enqueued upload may still read this slot's staging
    // done_ev lies behind every upload: once it has passed nothing is pending, and only otherwise
    // does a second open of the slot wait on the host
    if (hipEventQuery(p->done_ev) != hipSuccess) {
      (void)hipGetLastError();  // (hipErrorNotReady is not an error of ours)
      rc = quiesce(p);
      if (rc) return rc;
    }
    std::fill(p->tp_dirty.begin(), p->tp_dirty.end(), 0);
  }
  float2 *stage = p->tp_pin + (size_t)slot * p->tp_len;
  rc = zfft_tap_table(freq_word, n_taps, h, (float *)stage);
  if (rc) return rc;
  rc = use_stream(p, p->stream);  // behind the enqueued pushes, which may still read the row
  if (rc) return rc;
  hipError_t e = hipMemcpyAsync(p->tp_tab.as<float2>() + (size_t)slot * p->tp_len, stage,
                                (size_t)n_taps * sizeof(float2), hipMemcpyHostToDevice, p->stream);
  if (e != hipSuccess) return hip_fail(e, "tap table upload");
  p->tp_dirty[slot] = 1;
  zfft_plan::TapSlot &t = p->tp_slots[slot];
  t.open = true, t.fw = freq_word, t.D = decim, t.T = n_taps, t.n_open = p->tp_n;
  return done_on(p, p->stream);
}

int zfft_tap_close(zfft_plan *p, int32_t slot) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (!rc) rc = need_slot(p, slot);
  if (rc) return rc;
  if (!p->tp_slots[slot].open) return fail(ZFFT_EINVAL, "tap_close: the slot is not open");
  p->tp_slots[slot].open = false;  // (an enqueued push has its items by value)
  return ZFFT_OK;
}

int zfft_tap_info(const zfft_plan *p, int32_t slot, int32_t *is_open, int64_t *freq_word, int32_t *decim,
                  int32_t *n_taps, uint64_t *n_open, double *group_delay) {
  if (!p || !is_open || !freq_word || !decim || !n_taps || !n_open || !group_delay)
    return fail(ZFFT_EINVAL, "null argument");
  int rc = need_on(p);
  if (!rc) rc = need_slot(p, slot);
  if (rc) return rc;
  const zfft_plan::TapSlot &t = p->tp_slots[slot];
  *is_open = t.open;
  *freq_word = t.open ? t.fw : 0, *decim = t.open ? t.D : 0, *n_taps = t.open ? t.T : 0;
  *n_open = t.open ? t.n_open : 0;
  *group_delay = t.open ? 0.5 * (t.T - 1) : 0.0;
  return ZFFT_OK;
}

int zfft_tap_counts(const zfft_plan *p, int64_t n_samples, int64_t *counts) {
  if (!p || !counts) return fail(ZFFT_EINVAL, "null argument");
  int rc = need_on(p);
  if (rc) return rc;
  if (n_samples < 0 || n_samples > kTapMaxPush) return fail(ZFFT_EINVAL, "tap_counts: n_samples in [0, 2^31 - 1]");
  for (int s = 0; s < p->tp_max; ++s) {
    const zfft_plan::TapSlot &t = p->tp_slots[s];
    counts[s] = t.open ? tap_count(p->tp_n, t.n_open, n_samples, t.D) : 0;
  }
  return ZFFT_OK;
}

int zfft_tap_push_device(zfft_plan *p, const void *d_iq, int64_t n_samples, void *d_out, void *hip_stream) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  if (n_samples == 0) return ZFFT_OK;
  rc = check_push(p, n_samples);
  if (rc) return rc;
  if (!d_iq) return fail(ZFFT_EINVAL, "tap push: null input");
  TapOpen taps[kTapMaxTaps];
  TapItems items;
  const int ntaps = open_taps(p, taps);
  const TapForm f = choose_tap(p->tp_n, n_samples, p->tp_len, taps, ntaps, &items, p->tp_layout);
  if (!f.ok()) return fail(ZFFT_EINTERNAL, "tap push: no form for this call");
  if (f.total > 0 && !d_out) return fail(ZFFT_EINVAL, "tap push: null output");
  hipStream_t st = pick_stream(p, hip_stream);
  rc = use_stream(p, st);
  if (rc) return rc;
  p->n_marks = 0;
  mark(p, st, "start");
  hipError_t e = launch_tap_push(d_iq, p->cfg.in_dtype, n_samples, p->tp_len, f, items, p->tp_tab.as<float2>(),
                                 carry(p, p->tp_par), carry(p, p->tp_par ^ 1), (float2 *)d_out, st);
  if (e != hipSuccess) return hip_fail(e, "tap_push");
  mark(p, st, "tap_push");
  p->tp_n += (uint64_t)n_samples;
  p->tp_par ^= 1;
  return done_on(p, st);
}

int zfft_tap_push(zfft_plan *p, const void *iq, int64_t n_samples, void *out, int64_t *counts_out) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  if (n_samples < 0 || n_samples > kTapMaxPush) return fail(ZFFT_EINVAL, "tap push: n_samples in [0, 2^31 - 1]");
  std::vector<int64_t> counts((size_t)p->tp_max);
  rc = zfft_tap_counts(p, n_samples, counts.data());
  if (rc) return rc;
  if (counts_out) std::copy(counts.begin(), counts.end(), counts_out);
  if (n_samples == 0) return ZFFT_OK;
  rc = check_push(p, n_samples);
  if (rc) return rc;
  int64_t total = 0;
  for (int64_t c : counts) total += c;
  if (!iq || (total > 0 && !out)) return fail(ZFFT_EINVAL, "tap push: null host pointer");
  const size_t in_bytes = ((size_t)n_samples * in_elem_bytes(p->cfg.in_dtype) + 15) & ~(size_t)15;
  const size_t out_bytes = (size_t)total * sizeof(float2);
  rc = grow(p, p->tp_stage, in_bytes + out_bytes, "tap staging");
  if (!rc) rc = use_stream(p, p->stream);  // the staging may still be read by the previous call
  if (rc) return rc;
  char *d = p->tp_stage.as<char>();
  hipError_t e = hipMemcpyAsync(d, iq, (size_t)n_samples * in_elem_bytes(p->cfg.in_dtype), hipMemcpyHostToDevice,
                                p->stream);
  if (e != hipSuccess) return hip_fail(e, "H2D samples");
  rc = zfft_tap_push_device(p, d, n_samples, d + in_bytes, p->stream);
  if (rc) return rc;
  e = out_bytes ? hipMemcpyAsync(out, d + in_bytes, out_bytes, hipMemcpyDeviceToHost, p->stream) : hipSuccess;
  rc = sync_read(p, e, "tap push");
  if (!rc) std::fill(p->tp_dirty.begin(), p->tp_dirty.end(), 0);  // every upload has run
  return rc;
}

int zfft_tap_state(zfft_plan *p, uint64_t *samples_seen) {
  if (!p || !samples_seen) return fail(ZFFT_EINVAL, "null argument");
  int rc = need_on(p);
  if (rc) return rc;
  *samples_seen = p->tp_n;
  return ZFFT_OK;
}

int zfft_tap_reset(zfft_plan *p, int64_t n0) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  if (n0 < 0 || (uint64_t)n0 > kTapMaxCount) return fail(ZFFT_EINVAL, "tap_reset: n0 in [0, 2^62]");
  return restart(p, (uint64_t)n0);
}

}  // extern "C"
