// zfft_demod.cpp -- the demodulator bank of libzfft.so: AM, FM, SSB and power audio out of K
// complex baseband streams on the device (C-ABI and rule: zfft.h; kernel: demod_kernels.hip; form
// chooser and output counts: zfft_demod_plan.h).  The model is zfft_chan.cpp's:
// nothing runs inside zfft_process*, the step count is the host's, and the state on the device is
// the audio taps, a (mode, bfo_word) pair per stream and two alternating carries.  A mode change
// is one small launch on the plan's stream, so it needs no host memory that outlives the call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "zfft.h"
#include "zfft_demod_plan.h"
#include "zfft_plan.h"

using namespace zfft;

namespace zfft {

struct DemodState {
  int K = 0, Ta = 0, Da = 0;
  int par = 0;     // a push reads the carry of this parity and writes the other
  uint64_t n = 0;  // steps given (host side: pushes are in call order)
  DevBuf g, modes, carry, stage;  // Ta floats; K (mode, word) pairs; two carries of Ta K samples; zfft_demod_push's staging
};

void demod_release(zfft_plan *p) {
  delete p->demod;
  p->demod = nullptr;
}

}  // namespace zfft

namespace {

int need_on(const zfft_plan *p) { return p->demod ? ZFFT_OK : fail(ZFFT_EINVAL, "demod is off (zfft_plan_demod)"); }

size_t carry_len(const DemodState *d) { return (size_t)d->Ta * (size_t)d->K; }
float2 *carry(const DemodState *d, int par) { return d->carry.as<float2>() + (size_t)par * carry_len(d); }

int check_push(const DemodState *d, int64_t steps, int64_t step_stride, int64_t stream_stride) {
  if (steps < 1 || steps > kDemodMaxPush) return fail(ZFFT_EINVAL, "demod push: steps in [0, 2^31 - 1]");
  if (d->n + (uint64_t)steps > kDemodMaxCount) return fail(ZFFT_EINVAL, "demod push: the step count would pass 2^62");
  if (!demod_strides_ok(d->K, step_stride, stream_stride))
    return fail(ZFFT_EINVAL, "demod push: step_stride in [1, 2^31], stream_stride in [1, 2^31] (one stream: [0, 2^31])");
  return ZFFT_OK;
}

// The count back to n0 and the carry to zeros, in stream order on the plan's stream.
int restart(zfft_plan *p, uint64_t n0) {
  DemodState *d = p->demod;
  int rc = use_stream(p, p->stream);
  if (rc) return rc;
  hipError_t e = hipMemsetAsync(d->carry.p, 0, 2 * carry_len(d) * sizeof(float2), p->stream);
  if (e != hipSuccess) return hip_fail(e, "demod reset");
  d->n = n0;
  d->par = 0;
  return done_on(p, p->stream);
}

}  // namespace

extern "C" {

int zfft_plan_demod(zfft_plan *p, int32_t n_streams, int32_t n_taps, int32_t decim, const float *g) {
  int rc = enter(p);
  if (rc) return rc;
  if (n_streams == 0) {
    rc = quiesce(p);  // an enqueued push may still use all of it
    if (rc) return rc;
    demod_release(p);
    return ZFFT_OK;
  }
  if (!g)  // the default design has 8 decim + 1 taps
    n_taps = decim >= 1 && decim <= kDemodMaxDecim && (n_taps == 0 || n_taps == 8 * decim + 1) ? 8 * decim + 1 : -1;
  if (!demod_shape_ok(n_streams, n_taps, decim))
    return fail(ZFFT_EINVAL,
                "demod: n_streams in [1, 1024], n_taps in [1, 1024] (without taps: 0 or 8 decim + 1), decim in "
                "[1, 64]; or n_streams = 0 (off)");
  const int K = n_streams, Ta = n_taps;
  std::vector<float> gf((size_t)Ta);
  if (g) {
    std::copy(g, g + Ta, gf.begin());
  } else {
    std::vector<double> gd((size_t)Ta);
    rc = zfft_demod_design(Ta, 0.4 / decim, 8.0, gd.data());
    if (rc) return rc;
    for (int k = 0; k < Ta; ++k) gf[k] = (float)gd[k];
  }
  rc = quiesce(p);
  if (rc) return rc;
  demod_release(p);
  DemodState *d = p->demod = new DemodState;
  d->K = K, d->Ta = Ta, d->Da = decim;
  hipError_t e = d->g.ensure((size_t)Ta * sizeof(float));
  if (e == hipSuccess) e = d->modes.ensure((size_t)K * 2 * sizeof(uint32_t));
  if (e == hipSuccess) e = d->carry.ensure(2 * carry_len(d) * sizeof(float2));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    demod_release(p);
    return fail(ZFFT_ENOMEM, "demod allocation failed");
  }
  // nothing of the plan's is enqueued (quiesce): plain copies, complete on return
  e = hipMemcpy(d->g.p, gf.data(), (size_t)Ta * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d->modes.p, 0, (size_t)K * 2 * sizeof(uint32_t));  // (ZFFT_DEMOD_AM, 0)
  if (e != hipSuccess) {
    demod_release(p);
    return hip_fail(e, "demod table upload");
  }
  static_assert(ZFFT_DEMOD_AM == 0, "a zeroed pair is AM");
  rc = restart(p, 0);
  if (rc) demod_release(p);
  return rc;
}

int zfft_demod_shape(const zfft_plan *p, int32_t *n_streams, int32_t *n_taps, int32_t *decim) {
  if (!p || !n_streams || !n_taps || !decim) return fail(ZFFT_EINVAL, "null argument");
  *n_streams = *n_taps = *decim = 0;
  int rc = need_on(p);
  if (rc) return rc;
  *n_streams = p->demod->K, *n_taps = p->demod->Ta, *decim = p->demod->Da;
  return ZFFT_OK;
}

int zfft_demod_mode(zfft_plan *p, int32_t s_first, int32_t s_count, int32_t mode, int64_t bfo_word) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  DemodState *d = p->demod;
  if (s_first < 0 || s_count < 1 || s_first >= d->K || s_count > d->K - s_first || mode < ZFFT_DEMOD_AM ||
      mode > ZFFT_DEMOD_POWER || bfo_word < -((int64_t)1 << 31) || bfo_word >= ((int64_t)1 << 31))
    return fail(ZFFT_EINVAL,
                "demod_mode: s_first in [0, n_streams), s_count in [1, n_streams - s_first], mode one of "
                "ZFFT_DEMOD_*, bfo_word in [-2^31, 2^31)");
  rc = use_stream(p, p->stream);  // behind the enqueued pushes, which still read the pairs
  if (rc) return rc;
  hipError_t e = launch_demod_mode(d->modes.as<uint32_t>(), s_first, s_count, (uint32_t)mode,
                                   (uint32_t)(uint64_t)bfo_word, p->stream);
  if (e != hipSuccess) return hip_fail(e, "demod_mode");
  return done_on(p, p->stream);
}

int zfft_demod_steps(const zfft_plan *p, int64_t steps, int64_t *outputs) {
  if (!p || !outputs) return fail(ZFFT_EINVAL, "null argument");
  int rc = need_on(p);
  if (rc) return rc;
  if (steps < 0 || steps > kDemodMaxPush) return fail(ZFFT_EINVAL, "demod_steps: steps in [0, 2^31 - 1]");
  *outputs = demod_steps(p->demod->n, steps, p->demod->Da);
  return ZFFT_OK;
}

int zfft_demod_push_device(zfft_plan *p, const void *d_x, int64_t steps, int64_t step_stride, int64_t stream_stride,
                           void *d_out, void *hip_stream) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  if (steps == 0) return ZFFT_OK;
  DemodState *d = p->demod;
  rc = check_push(d, steps, step_stride, stream_stride);
  if (rc) return rc;
  if (!d_x) return fail(ZFFT_EINVAL, "demod push: null input");
  if (((uintptr_t)d_x & 7) || ((uintptr_t)d_out & 3)) return fail(ZFFT_EINVAL, "demod push: misaligned pointer");
  const DemodForm f = choose_demod(d->K, d->Ta, d->Da, step_stride, stream_stride);
  const DemodCut c = demod_cut(f, d->n, steps, d->Da);
  if (!f.ok() || !c.ok()) return fail(ZFFT_EINTERNAL, "demod push: no form for this call");
  if (c.outs > 0 && !d_out) return fail(ZFFT_EINVAL, "demod push: null output");
  hipStream_t st = pick_stream(p, hip_stream);
  rc = use_stream(p, st);
  if (rc) return rc;
  p->n_marks = 0;
  mark(p, st, "start");
  hipError_t e = launch_demod_push((const float2 *)d_x, steps, step_stride, stream_stride, d->n, d->K, d->Ta, d->Da, f, c,
                                   d->g.as<float>(), d->modes.as<uint32_t>(), carry(d, d->par), carry(d, d->par ^ 1),
                                   (float *)d_out, st);
  if (e != hipSuccess) return hip_fail(e, "demod_push");
  mark(p, st, "demod_push");
  d->n += (uint64_t)steps;
  d->par ^= 1;
  return done_on(p, st);
}

int zfft_demod_push(zfft_plan *p, const void *x, int64_t steps, int64_t step_stride, int64_t stream_stride, void *out,
                    int64_t *outputs_out) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  int64_t outs = 0;
  rc = zfft_demod_steps(p, steps, &outs);
  if (rc) return rc;
  if (outputs_out) *outputs_out = outs;
  if (steps == 0) return ZFFT_OK;
  DemodState *d = p->demod;
  rc = check_push(d, steps, step_stride, stream_stride);
  if (rc) return rc;
  if (!x || (outs > 0 && !out)) return fail(ZFFT_EINVAL, "demod push: null host pointer");
  const size_t count = (size_t)(steps - 1) * (size_t)step_stride + (size_t)(d->K - 1) * (size_t)stream_stride + 1;
  const size_t in_bytes = (count * sizeof(float2) + 15) & ~(size_t)15;
  const size_t out_bytes = (size_t)outs * (size_t)d->K * sizeof(float);
  rc = grow(p, d->stage, in_bytes + out_bytes, "demod staging");
  if (!rc) rc = use_stream(p, p->stream);  // the staging may still be read by the previous call
  if (rc) return rc;
  char *dev = d->stage.as<char>();
  hipError_t e = hipMemcpyAsync(dev, x, count * sizeof(float2), hipMemcpyHostToDevice, p->stream);
  if (e != hipSuccess) return hip_fail(e, "H2D samples");
  rc = zfft_demod_push_device(p, dev, steps, step_stride, stream_stride, dev + in_bytes, p->stream);
  if (rc) return rc;
  e = out_bytes ? hipMemcpyAsync(out, dev + in_bytes, out_bytes, hipMemcpyDeviceToHost, p->stream) : hipSuccess;
  return sync_read(p, e, "demod push");
}

int zfft_demod_state(zfft_plan *p, uint64_t *steps_seen) {
  if (!p || !steps_seen) return fail(ZFFT_EINVAL, "null argument");
  int rc = need_on(p);
  if (rc) return rc;
  *steps_seen = p->demod->n;
  return ZFFT_OK;
}

int zfft_demod_reset(zfft_plan *p, int64_t n0) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  if (n0 < 0 || (uint64_t)n0 > kDemodMaxCount) return fail(ZFFT_EINVAL, "demod_reset: n0 in [0, 2^62]");
  return restart(p, (uint64_t)n0);
}

int zfft_demod_info(const zfft_plan *p, double *group_delay, double *rate_ratio) {
  if (!p || !group_delay || !rate_ratio) return fail(ZFFT_EINVAL, "null argument");
  int rc = need_on(p);
  if (rc) return rc;
  *group_delay = 0.5 * (p->demod->Ta - 1);
  *rate_ratio = 1.0 / p->demod->Da;
  return ZFFT_OK;
}

}  // extern "C"
