// zfft_demod.cpp -- the demodulator bank of libzfft.so: AM, FM, SSB and power audio out of K
// complex baseband streams on the device (C-ABI and rule: zfft.h; kernel: demod_kernels.hip; form
// chooser and output counts: zfft_demod_plan.h).  Nothing runs inside
// zfft_process*, the step count is the host's, and the state on the device is the audio taps, a
// (mode, bfo_word) pair per stream and two alternating carries.  Count, carries and the host push's
// staging go through the producers' shared path (zfft_stream.h).  A mode change is one small
// launch on the plan's stream, so it needs no host memory that outlives the call.
#include <algorithm>
#include <vector>

#include "zfft.h"
#include "zfft_demod_plan.h"
#include "zfft_stream.h"

using namespace zfft;

namespace zfft {

struct DemodState {
  int K = 0, Ta = 0, Da = 0;
  DevBuf g, modes;  // Ta floats; K (mode, word) pairs
  StreamState s;    // steps given; two carries of Ta K samples; zfft_demod_push's staging
};

void demod_release(zfft_plan *p) {
  delete p->demod;
  p->demod = nullptr;
}

}  // namespace zfft

namespace {

constexpr StreamNames kNames{"demod", "steps", "step"};

int need_on(const zfft_plan *p) { return p->demod ? ZFFT_OK : fail(ZFFT_EINVAL, "demod is off (zfft_plan_demod)"); }

int check_push(const DemodState *d, int64_t steps, int64_t step_stride, int64_t stream_stride) {
  int rc = stream_check_push(d->s, kNames, steps);
  if (rc) return rc;
  if (!demod_strides_ok(d->K, step_stride, stream_stride))
    return fail(ZFFT_EINVAL, "demod push: step_stride in [1, 2^31], stream_stride in [1, 2^31] (one stream: [0, 2^31])");
  return ZFFT_OK;
}

// A checked push of steps >= 1 from device memory, enqueued on the caller's stream.
int push_on(zfft_plan *p, const void *d_x, int64_t steps, int64_t step_stride, int64_t stream_stride, void *d_out,
            void *hip_stream) {
  DemodState *d = p->demod;
  if (!d_x) return fail(ZFFT_EINVAL, "demod push: null input");
  if (((uintptr_t)d_x & 7) || ((uintptr_t)d_out & 3)) return fail(ZFFT_EINVAL, "demod push: misaligned pointer");
  const DemodForm f = choose_demod(d->K, d->Ta, d->Da, step_stride, stream_stride);
  const DemodCut c = demod_cut(f, d->s.n, steps, d->Da);
  if (!f.ok() || !c.ok()) return fail(ZFFT_EINTERNAL, "demod push: no form for this call");
  if (c.outs > 0 && !d_out) return fail(ZFFT_EINVAL, "demod push: null output");
  hipStream_t st;
  int rc = begin_call(p, hip_stream, &st);
  if (rc) return rc;
  hipError_t e = launch_demod_push((const float2 *)d_x, steps, step_stride, stream_stride, d->s.n, d->K, d->Ta, d->Da, f, c,
                                   d->g.as<float>(), d->modes.as<uint32_t>(), d->s.carry_in(), d->s.carry_out(),
                                   (float *)d_out, st);
  if (e != hipSuccess) return hip_fail(e, "demod_push");
  mark(p, st, "demod_push");
  return stream_commit(p, d->s, steps, st);
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
  if (e == hipSuccess) e = stream_alloc(d->s, (size_t)Ta * (size_t)K);
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
  rc = stream_restart(p, d->s, kNames, 0);
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
  if (!rc) rc = need_on(p);
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
  *outputs = demod_steps(p->demod->s.n, steps, p->demod->Da);
  return ZFFT_OK;
}

int zfft_demod_push_device(zfft_plan *p, const void *d_x, int64_t steps, int64_t step_stride, int64_t stream_stride,
                           void *d_out, void *hip_stream) {
  int rc = enter(p);
  if (!rc) rc = need_on(p);
  if (rc || steps == 0) return rc;
  rc = check_push(p->demod, steps, step_stride, stream_stride);
  return rc ? rc : push_on(p, d_x, steps, step_stride, stream_stride, d_out, hip_stream);
}

int zfft_demod_push(zfft_plan *p, const void *x, int64_t steps, int64_t step_stride, int64_t stream_stride, void *out,
                    int64_t *outputs_out) {
  int rc = enter(p);
  if (!rc) rc = need_on(p);
  if (rc) return rc;
  int64_t outs = 0;
  rc = zfft_demod_steps(p, steps, &outs);
  if (rc) return rc;
  if (outputs_out) *outputs_out = outs;
  if (steps == 0) return ZFFT_OK;
  DemodState *d = p->demod;
  rc = check_push(d, steps, step_stride, stream_stride);
  if (rc) return rc;
  const size_t count = (size_t)(steps - 1) * (size_t)step_stride + (size_t)(d->K - 1) * (size_t)stream_stride + 1;
  return stream_host_push(p, d->s, kNames, x, count * sizeof(float2), out, (size_t)outs * (size_t)d->K * sizeof(float),
                          [=](const void *d_in, void *d_out) {
                            return push_on(p, d_in, steps, step_stride, stream_stride, d_out, p->stream);
                          });
}

int zfft_demod_state(zfft_plan *p, uint64_t *steps_seen) {
  if (!p || !steps_seen) return fail(ZFFT_EINVAL, "null argument");
  int rc = need_on(p);
  if (!rc) *steps_seen = p->demod->s.n;
  return rc;
}

int zfft_demod_reset(zfft_plan *p, int64_t n0) {
  int rc = enter(p);
  if (!rc) rc = need_on(p);
  return rc ? rc : stream_reset(p, p->demod->s, kNames, n0);
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
