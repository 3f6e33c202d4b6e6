// zfft_chan.cpp -- the channeliser of libzfft.so: a polyphase-FFT bank of M uniform channels on
// the plan's input samples (C-ABI and rule: zfft.h; kernel: chan_kernels.hip; form chooser, step
// counts and the transform's layout: zfft_chan_plan.h).  Nothing runs
// inside zfft_process*, the sample count is the host's, and the state on the device is the
// prototype, the twiddles and two alternating carries.  Count, carries and the host push's staging
// go through the producers' shared path (zfft_stream.h) and are its own: the taps neither see nor
// move them.
#include <algorithm>
#include <vector>

#include "zfft.h"
#include "zfft_chan_plan.h"
#include "zfft_stream.h"

using namespace zfft;

namespace zfft {

struct ChanState {
  int M = 0, P = 0, D = 0;
  int c_first = 0, c_count = 0;
  DevBuf h, tw;    // M P floats; M float2
  StreamState s;   // samples given; two carries of M P - 1 samples; zfft_chan_push's staging
};

void chan_release(zfft_plan *p) {
  delete p->chan;
  p->chan = nullptr;
}

}  // namespace zfft

namespace {

constexpr StreamNames kNames{"chan", "n_samples", "sample"};

int need_on(const zfft_plan *p) { return p->chan ? ZFFT_OK : fail(ZFFT_EINVAL, "channels are off (zfft_plan_chan)"); }

// A checked push of n_samples >= 1 from device memory, enqueued on the caller's stream.
int push_on(zfft_plan *p, const void *d_iq, int64_t n_samples, void *d_out, void *hip_stream) {
  ChanState *c = p->chan;
  if (!d_iq) return fail(ZFFT_EINVAL, "chan push: null input");
  const ChanForm f = choose_chan(c->s.n, n_samples, c->M, c->P, c->D, c->c_count);
  if (!f.ok()) return fail(ZFFT_EINTERNAL, "chan push: no form for this call");
  if (f.steps > 0 && !d_out) return fail(ZFFT_EINVAL, "chan push: null output");
  hipStream_t st;
  int rc = begin_call(p, hip_stream, &st);
  if (rc) return rc;
  hipError_t e = launch_chan_push(d_iq, p->cfg.in_dtype, n_samples, c->M, c->P, c->D, c->c_first, c->c_count, f,
                                  c->h.as<float>(), c->tw.as<float2>(), c->s.carry_in(), c->s.carry_out(),
                                  (float2 *)d_out, st);
  if (e != hipSuccess) return hip_fail(e, "chan_push");
  mark(p, st, "chan_push");
  return stream_commit(p, c->s, n_samples, st);
}

}  // namespace

extern "C" {

int zfft_plan_chan(zfft_plan *p, int32_t n_chan, int32_t taps_per_chan, int32_t decim, const float *h) {
  int rc = enter(p);
  if (rc) return rc;
  if (n_chan == 0) {
    rc = quiesce(p);  // an enqueued push may still use all of it
    if (rc) return rc;
    chan_release(p);
    return ZFFT_OK;
  }
  if (!chan_shape_ok(n_chan, taps_per_chan, decim))
    return fail(ZFFT_EINVAL,
                "chan: n_chan a power of two in [8, 1024], taps_per_chan >= 1, n_chan taps_per_chan <= 2048, "
                "decim n_chan or n_chan / 2; or n_chan = 0 (off)");
  if (p->cfg.flip_input) return fail(ZFFT_EUNSUPPORTED, "chan: flip_input = 1 has no continuous time axis");
  const int M = n_chan, P = taps_per_chan, T = M * P;
  std::vector<float> hf((size_t)T), tw((size_t)2 * M);
  if (h) {
    std::copy(h, h + T, hf.begin());
  } else {
    std::vector<double> hd((size_t)T);
    rc = zfft_chan_design(M, P, 8.0, hd.data());
    if (rc) return rc;
    for (int k = 0; k < T; ++k) hf[k] = (float)hd[k];
  }
  chan_twiddles(M, tw.data());
  rc = quiesce(p);
  if (rc) return rc;
  chan_release(p);
  ChanState *c = p->chan = new ChanState;
  c->M = M, c->P = P, c->D = decim;
  c->c_first = 0, c->c_count = M;
  hipError_t e = c->h.ensure((size_t)T * sizeof(float));
  if (e == hipSuccess) e = c->tw.ensure((size_t)M * sizeof(float2));
  if (e == hipSuccess) e = stream_alloc(c->s, (size_t)(T - 1));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    chan_release(p);
    return fail(ZFFT_ENOMEM, "chan allocation failed");
  }
  // nothing of the plan's is enqueued (quiesce): plain copies, complete on return
  e = hipMemcpy(c->h.p, hf.data(), (size_t)T * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(c->tw.p, tw.data(), (size_t)M * sizeof(float2), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    chan_release(p);
    return hip_fail(e, "chan table upload");
  }
  rc = stream_restart(p, c->s, kNames, 0);
  if (rc) chan_release(p);
  return rc;
}

int zfft_chan_shape(const zfft_plan *p, int32_t *n_chan, int32_t *taps_per_chan, int32_t *decim, int32_t *c_first,
                    int32_t *c_count) {
  if (!p || !n_chan || !taps_per_chan || !decim || !c_first || !c_count) return fail(ZFFT_EINVAL, "null argument");
  *n_chan = *taps_per_chan = *decim = *c_first = *c_count = 0;
  int rc = need_on(p);
  if (rc) return rc;
  const ChanState *c = p->chan;
  *n_chan = c->M, *taps_per_chan = c->P, *decim = c->D, *c_first = c->c_first, *c_count = c->c_count;
  return ZFFT_OK;
}

int zfft_chan_select(zfft_plan *p, int32_t c_first, int32_t c_count) {
  int rc = enter(p);
  if (!rc) rc = need_on(p);
  if (rc) return rc;
  ChanState *c = p->chan;
  if (c_first < 0 || c_first >= c->M || c_count < 1 || c_count > c->M)
    return fail(ZFFT_EINVAL, "chan_select: c_first in [0, n_chan), c_count in [1, n_chan]");
  c->c_first = c_first, c->c_count = c_count;  // (an enqueued push has its selection by value)
  return ZFFT_OK;
}

int zfft_chan_steps(const zfft_plan *p, int64_t n_samples, int64_t *steps) {
  if (!p || !steps) return fail(ZFFT_EINVAL, "null argument");
  int rc = need_on(p);
  if (rc) return rc;
  if (n_samples < 0 || n_samples > kChanMaxPush) return fail(ZFFT_EINVAL, "chan_steps: n_samples in [0, 2^31 - 1]");
  *steps = chan_steps(p->chan->s.n, n_samples, p->chan->D);
  return ZFFT_OK;
}

int zfft_chan_push_device(zfft_plan *p, const void *d_iq, int64_t n_samples, void *d_out, void *hip_stream) {
  int rc = enter(p);
  if (!rc) rc = need_on(p);
  if (rc || n_samples == 0) return rc;
  rc = stream_check_push(p->chan->s, kNames, n_samples);
  return rc ? rc : push_on(p, d_iq, n_samples, d_out, hip_stream);
}

int zfft_chan_push(zfft_plan *p, const void *iq, int64_t n_samples, void *out, int64_t *steps_out) {
  int rc = enter(p);
  if (!rc) rc = need_on(p);
  if (rc) return rc;
  int64_t steps = 0;
  rc = zfft_chan_steps(p, n_samples, &steps);
  if (rc) return rc;
  if (steps_out) *steps_out = steps;
  if (n_samples == 0) return ZFFT_OK;
  ChanState *c = p->chan;
  rc = stream_check_push(c->s, kNames, n_samples);
  if (rc) return rc;
  return stream_host_push(p, c->s, kNames, iq, (size_t)n_samples * in_elem_bytes(p->cfg.in_dtype), out,
                          (size_t)steps * (size_t)c->c_count * sizeof(float2),
                          [=](const void *d_in, void *d_out) { return push_on(p, d_in, n_samples, d_out, p->stream); });
}

int zfft_chan_state(zfft_plan *p, uint64_t *samples_seen) {
  if (!p || !samples_seen) return fail(ZFFT_EINVAL, "null argument");
  int rc = need_on(p);
  if (!rc) *samples_seen = p->chan->s.n;
  return rc;
}

int zfft_chan_reset(zfft_plan *p, int64_t n0) {
  int rc = enter(p);
  if (!rc) rc = need_on(p);
  return rc ? rc : stream_reset(p, p->chan->s, kNames, n0);
}

int zfft_chan_info(const zfft_plan *p, double *group_delay, double *rate_ratio) {
  if (!p || !group_delay || !rate_ratio) return fail(ZFFT_EINVAL, "null argument");
  int rc = need_on(p);
  if (rc) return rc;
  *group_delay = 0.5 * (p->chan->M * p->chan->P - 1);
  *rate_ratio = 1.0 / p->chan->D;
  return ZFFT_OK;
}

}  // extern "C"
