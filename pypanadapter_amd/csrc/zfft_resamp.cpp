// zfft_resamp.cpp -- the resampler bank of libzfft.so: K real float32 lanes on the device at L / M
// times their rate, as float32 or int16 (C-ABI and rule: zfft.h; kernel: resamp_kernels.hip; form
// chooser and output counts: zfft_resamp_plan.h).  Nothing runs inside
// zfft_process*, the step count is the host's, and the state on the device is the phase-major
// coefficient table and two alternating carries of T - 1 steps.  Count, carries and the host
// push's staging go through the producers' shared path (zfft_stream.h), whose carries are float2
// arrays: each is sized to ceil((T - 1) K / 2) of them and used as floats.
#include <algorithm>
#include <vector>

#include "zfft.h"
#include "zfft_resamp_plan.h"
#include "zfft_stream.h"

using namespace zfft;

namespace zfft {

struct ResampState {
  int K = 0, L = 0, M = 0, T = 0, format = 0;
  float scale = 0.f;
  DevBuf hp;      // hp[phase][k] = h[k L + phase], L T floats
  StreamState s;  // steps given; two carries of (T - 1) K floats; zfft_resamp_push's staging
};

void resamp_release(zfft_plan *p) {
  delete p->resamp;
  p->resamp = nullptr;
}

}  // namespace zfft

namespace {

constexpr StreamNames kNames{"resamp", "steps", "step"};

int need_on(const zfft_plan *p) { return p->resamp ? ZFFT_OK : fail(ZFFT_EINVAL, "resamp is off (zfft_plan_resamp)"); }

size_t out_size(const ResampState *r) { return r->format == ZFFT_RESAMP_S16 ? sizeof(int16_t) : sizeof(float); }

int check_push(const ResampState *r, int64_t steps, int64_t step_stride) {
  int rc = stream_check_push(r->s, kNames, steps);
  if (rc) return rc;
  if (!resamp_stride_ok(r->K, step_stride)) return fail(ZFFT_EINVAL, "resamp push: step_stride in [n_lanes, 2^31]");
  return ZFFT_OK;
}

// A checked push of steps >= 1 from device memory, enqueued on the caller's stream.
int push_on(zfft_plan *p, const void *d_x, int64_t steps, int64_t step_stride, void *d_out, void *stream) {
  ResampState *r = p->resamp;
  if (!d_x) return fail(ZFFT_EINVAL, "resamp push: null input");
  if (((uintptr_t)d_x & 3) || ((uintptr_t)d_out & (out_size(r) - 1))) return fail(ZFFT_EINVAL, "resamp push: misaligned pointer");
  const ResampForm f = choose_resamp(r->K, r->L, r->M, r->T, step_stride, r->format);
  const ResampCut c = resamp_cut(f, r->s.n, steps);
  if (!f.ok() || !c.ok()) return fail(ZFFT_EINTERNAL, "resamp push: no form for this call");
  if (c.outs > 0 && !d_out) return fail(ZFFT_EINVAL, "resamp push: null output");
  hipStream_t st;
  int rc = begin_call(p, stream, &st);
  if (rc) return rc;
  hipError_t e = launch_resamp_push((const float *)d_x, steps, step_stride, f, c, r->format, r->scale, r->hp.as<float>(),
                                    (const float *)r->s.carry_in(), (float *)r->s.carry_out(), d_out, st);
  if (e != hipSuccess) return hip_fail(e, "resamp_push");
  mark(p, st, "resamp_push");
  return stream_commit(p, r->s, steps, st);
}

}  // namespace

extern "C" {

int zfft_plan_resamp(zfft_plan *p, int32_t n_lanes, int32_t L, int32_t M, int32_t taps_per_phase, const float *h,
                     int32_t format, float scale) {
  int rc = enter(p);
  if (rc) return rc;
  if (n_lanes == 0) {
    rc = quiesce(p);  // an enqueued push may still use all of it
    if (rc) return rc;
    resamp_release(p);
    return ZFFT_OK;
  }
  if (!h) {  // the default design has 16 ceil(max(L, M) / L) taps a phase
    const int T = L >= 1 && L <= kResampMaxL && M >= 1 && M <= kResampMaxM ? 16 * ((std::max(L, M) + L - 1) / L) : -1;
    taps_per_phase = taps_per_phase == 0 || taps_per_phase == T ? T : -1;
  }
  if (!resamp_shape_ok(n_lanes, L, M, taps_per_phase) || (format != ZFFT_RESAMP_F32 && format != ZFFT_RESAMP_S16))
    return fail(ZFFT_EINVAL,
                "resamp: n_lanes in [1, 2048], L in [1, 512], M in [1, 4096], gcd(L, M) = 1, taps_per_phase in [1, 128] "
                "(without taps: 0 or 16 ceil(max(L, M) / L)), L taps_per_phase <= 8192, format ZFFT_RESAMP_F32 or "
                "ZFFT_RESAMP_S16; or n_lanes = 0 (off)");
  const int K = n_lanes, T = taps_per_phase;
  std::vector<float> hp((size_t)L * T);
  if (h) {
    for (int ph = 0; ph < L; ++ph)
      for (int k = 0; k < T; ++k) hp[(size_t)ph * T + k] = h[(size_t)k * L + ph];
  } else {
    std::vector<double> hd((size_t)L * T);
    rc = zfft_resamp_design(L, M, T, 8.0, hd.data());
    if (rc) return rc;
    for (int ph = 0; ph < L; ++ph)
      for (int k = 0; k < T; ++k) hp[(size_t)ph * T + k] = (float)hd[(size_t)k * L + ph];
  }
  rc = quiesce(p);
  if (rc) return rc;
  resamp_release(p);
  ResampState *r = p->resamp = new ResampState;
  r->K = K, r->L = L, r->M = M, r->T = T, r->format = format, r->scale = scale;
  hipError_t e = r->hp.ensure(hp.size() * sizeof(float));
  // (T = 1 carries nothing: one float2 stands in, so that the carries are always memory)
  if (e == hipSuccess) e = stream_alloc(r->s, std::max<size_t>(1, ((size_t)(T - 1) * (size_t)K + 1) / 2));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    resamp_release(p);
    return fail(ZFFT_ENOMEM, "resamp allocation failed");
  }
  // nothing of the plan's is enqueued (quiesce): a plain copy, complete on return
  e = hipMemcpy(r->hp.p, hp.data(), hp.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    resamp_release(p);
    return hip_fail(e, "resamp table upload");
  }
  rc = stream_restart(p, r->s, kNames, 0);
  if (rc) resamp_release(p);
  return rc;
}

int zfft_resamp_shape(const zfft_plan *p, int32_t *n_lanes, int32_t *L, int32_t *M, int32_t *taps_per_phase,
                      int32_t *format) {
  if (!p || !n_lanes || !L || !M || !taps_per_phase || !format) return fail(ZFFT_EINVAL, "null argument");
  *n_lanes = *L = *M = *taps_per_phase = *format = 0;
  int rc = need_on(p);
  if (rc) return rc;
  const ResampState *r = p->resamp;
  *n_lanes = r->K, *L = r->L, *M = r->M, *taps_per_phase = r->T, *format = r->format;
  return ZFFT_OK;
}

int zfft_resamp_steps(const zfft_plan *p, int64_t steps, int64_t *outputs) {
  if (!p || !outputs) return fail(ZFFT_EINVAL, "null argument");
  int rc = need_on(p);
  if (rc) return rc;
  if (steps < 0 || steps > kResampMaxPush) return fail(ZFFT_EINVAL, "resamp_steps: steps in [0, 2^31 - 1]");
  *outputs = resamp_steps(p->resamp->s.n, steps, p->resamp->L, p->resamp->M);
  return ZFFT_OK;
}

int zfft_resamp_push_device(zfft_plan *p, const void *d_x, int64_t steps, int64_t step_stride, void *d_out, void *stream) {
  int rc = enter(p);
  if (!rc) rc = need_on(p);
  if (rc || steps == 0) return rc;
  rc = check_push(p->resamp, steps, step_stride);
  return rc ? rc : push_on(p, d_x, steps, step_stride, d_out, stream);
}

int zfft_resamp_push(zfft_plan *p, const void *x, int64_t steps, int64_t step_stride, void *out, int64_t *outputs_out) {
  int rc = enter(p);
  if (!rc) rc = need_on(p);
  if (rc) return rc;
  int64_t outs = 0;
  rc = zfft_resamp_steps(p, steps, &outs);
  if (rc) return rc;
  if (outputs_out) *outputs_out = outs;
  if (steps == 0) return ZFFT_OK;
  ResampState *r = p->resamp;
  rc = check_push(r, steps, step_stride);
  if (rc) return rc;
  const size_t count = (size_t)(steps - 1) * (size_t)step_stride + (size_t)r->K;
  return stream_host_push(p, r->s, kNames, x, count * sizeof(float), out, (size_t)outs * (size_t)r->K * out_size(r),
                          [=](const void *d_in, void *d_out) { return push_on(p, d_in, steps, step_stride, d_out, p->stream); });
}

int zfft_resamp_state(zfft_plan *p, uint64_t *steps_seen) {
  if (!p || !steps_seen) return fail(ZFFT_EINVAL, "null argument");
  int rc = need_on(p);
  if (!rc) *steps_seen = p->resamp->s.n;
  return rc;
}

int zfft_resamp_reset(zfft_plan *p, int64_t n0) {
  int rc = enter(p);
  if (!rc) rc = need_on(p);
  return rc ? rc : stream_reset(p, p->resamp->s, kNames, n0);
}

int zfft_resamp_info(const zfft_plan *p, double *group_delay, double *rate_ratio) {
  if (!p || !group_delay || !rate_ratio) return fail(ZFFT_EINVAL, "null argument");
  int rc = need_on(p);
  if (rc) return rc;
  const ResampState *r = p->resamp;
  *group_delay = ((double)r->T * r->L - 1.0) / (2.0 * r->L);
  *rate_ratio = (double)r->L / r->M;
  return ZFFT_OK;
}

}  // extern "C"
