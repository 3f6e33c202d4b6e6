// zfft_level.cpp -- the level bank of libzfft.so: look-ahead gain control and squelch on K real
// float32 lanes on the device (C-ABI and rule: zfft.h; kernels: level_kernels.hip; form chooser,
// emitted() and the block ranges of a push: zfft_level_plan.h).  Nothing runs
// inside zfft_process*, the step count is the host's, and the state on the device is two
// alternating carries -- the unemitted steps, the running peaks and the last H + 2 block peaks --
// and two grow-only work arrays of a push, its block peaks and block gains.  Count, carries and
// the host push's staging go through the producers' shared path (zfft_stream.h), whose carries are
// float2 arrays: each is sized to ceil((2 B + H + 2) K / 2) of them and used as floats.
#include <algorithm>
#include <vector>

#include "zfft.h"
#include "zfft_level_plan.h"
#include "zfft_stream.h"

using namespace zfft;

namespace zfft {

struct LevelState {
  int K = 0, B = 0, H = 0;
  float par[4] = {};  // target, gmax, floor, squelch
  uint64_t n_r = 0;   // the count the bank was started at (rule 2)
  DevBuf pk, gk;      // a push's block peaks (npk K floats) and block gains (nq K floats)
  StreamState s;      // steps given; two carries of (2 B + H + 2) K floats; zfft_level_push's staging
};

void level_release(zfft_plan *p) {
  delete p->level;
  p->level = nullptr;
}

}  // namespace zfft

namespace {

constexpr StreamNames kNames{"level", "steps", "step"};

int need_on(const zfft_plan *p) { return p->level ? ZFFT_OK : fail(ZFFT_EINVAL, "level is off (zfft_plan_level)"); }

int check_push(const LevelState *r, int64_t steps, int64_t step_stride, bool keyed, int64_t key_stride) {
  int rc = stream_check_push(r->s, kNames, steps);
  if (rc) return rc;
  if (!level_stride_ok(r->K, step_stride)) return fail(ZFFT_EINVAL, "level push: step_stride in [n_lanes, 2^31]");
  if (keyed && !level_stride_ok(r->K, key_stride)) return fail(ZFFT_EINVAL, "level push: key_stride in [n_lanes, 2^31]");
  return ZFFT_OK;
}

// A checked push of steps >= 1 from device memory, enqueued on the caller's stream.
int push_on(zfft_plan *p, const void *d_x, int64_t steps, int64_t step_stride, const void *d_key, int64_t key_stride,
            void *d_out, void *stream) {
  LevelState *r = p->level;
  if (!d_x) return fail(ZFFT_EINVAL, "level push: null input");
  if (((uintptr_t)d_x & 3) || ((uintptr_t)d_key & 3) || ((uintptr_t)d_out & 3)) return fail(ZFFT_EINVAL, "level push: misaligned pointer");
  if (!d_key) d_key = d_x, key_stride = step_stride;
  const LevelForm f = choose_level(r->K, r->B, r->H);
  const LevelCut c = level_cut(f, r->s.n, r->n_r, steps);
  if (!f.ok() || !c.ok()) return fail(ZFFT_EINTERNAL, "level push: no form for this call");
  if (c.outs > 0 && !d_out) return fail(ZFFT_EINVAL, "level push: null output");
  if (c.outs > 0 && (d_out == d_x || d_out == d_key)) return fail(ZFFT_EINVAL, "level push: the output overlaps an input");
  // (a longer push than any before: the work arrays grow, after a wait for what may still read them)
  int rc = grow(p, r->pk, (size_t)c.npk * (size_t)r->K * sizeof(float), "level peaks");
  if (!rc) rc = grow(p, r->gk, (size_t)c.nq * (size_t)r->K * sizeof(float), "level gains");
  if (rc) return rc;
  hipStream_t st;
  rc = begin_call(p, stream, &st);
  if (rc) return rc;
  const float *old = (const float *)r->s.carry_in();
  float *next = (float *)r->s.carry_out();
  hipError_t e = launch_level_peaks((const float *)d_key, key_stride, f, c, old, next, r->pk.as<float>(), st);
  if (e != hipSuccess) return hip_fail(e, "level_peaks");
  mark(p, st, "level_peaks");
  if (c.outs > 0) {
    e = launch_level_gains(f, c, r->par, r->pk.as<float>(), r->gk.as<float>(), st);
    if (e != hipSuccess) return hip_fail(e, "level_gains");
    mark(p, st, "level_gains");
  }
  e = launch_level_apply((const float *)d_x, step_stride, f, c, old, next, r->pk.as<float>(), r->gk.as<float>(), (float *)d_out, st);
  if (e != hipSuccess) return hip_fail(e, "level_apply");
  mark(p, st, "level_apply");
  return stream_commit(p, r->s, steps, st);
}

}  // namespace

extern "C" {

int zfft_plan_level(zfft_plan *p, int32_t n_lanes, int32_t block, int32_t hold, float target, float gmax, float floor,
                    float squelch) {
  int rc = enter(p);
  if (rc) return rc;
  if (n_lanes == 0) {
    rc = quiesce(p);  // an enqueued push may still use all of it
    if (rc) return rc;
    level_release(p);
    return ZFFT_OK;
  }
  if (!level_shape_ok(n_lanes, block, hold) || !level_params_ok(target, gmax, floor, squelch))
    return fail(ZFFT_EINVAL,
                "level: n_lanes in [1, 2048], block a power of two in [8, 1024], hold in [0, 4096], target, gmax and "
                "floor in [2^-60, 2^60], squelch 0 or in [2^-60, 2^60]; or n_lanes = 0 (off)");
  rc = quiesce(p);
  if (rc) return rc;
  level_release(p);
  LevelState *r = p->level = new LevelState;
  r->K = n_lanes, r->B = block, r->H = hold;
  r->par[0] = target, r->par[1] = gmax, r->par[2] = floor, r->par[3] = squelch;
  // the work arrays of a push that completes no block, so that they are always memory
  hipError_t e = stream_alloc(r->s, (level_carry_floats(r->K, r->B, r->H) + 1) / 2);
  if (e == hipSuccess) e = r->pk.ensure((size_t)(hold + 2) * (size_t)n_lanes * sizeof(float));
  if (e == hipSuccess) e = r->gk.ensure((size_t)2 * (size_t)n_lanes * sizeof(float));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    level_release(p);
    return fail(ZFFT_ENOMEM, "level allocation failed");
  }
  r->n_r = 0;
  rc = stream_restart(p, r->s, kNames, 0);
  if (rc) level_release(p);
  return rc;
}

int zfft_level_shape(const zfft_plan *p, int32_t *n_lanes, int32_t *block, int32_t *hold, float *target, float *gmax,
                     float *floor, float *squelch) {
  if (!p || !n_lanes || !block || !hold || !target || !gmax || !floor || !squelch) return fail(ZFFT_EINVAL, "null argument");
  *n_lanes = *block = *hold = 0;
  *target = *gmax = *floor = *squelch = 0.f;
  int rc = need_on(p);
  if (rc) return rc;
  const LevelState *r = p->level;
  *n_lanes = r->K, *block = r->B, *hold = r->H;
  *target = r->par[0], *gmax = r->par[1], *floor = r->par[2], *squelch = r->par[3];
  return ZFFT_OK;
}

int zfft_level_steps(const zfft_plan *p, int64_t steps, int64_t *outputs) {
  if (!p || !outputs) return fail(ZFFT_EINVAL, "null argument");
  int rc = need_on(p);
  if (rc) return rc;
  if (steps < 0 || steps > kLevelMaxPush) return fail(ZFFT_EINVAL, "level_steps: steps in [0, 2^31 - 1]");
  *outputs = level_steps(p->level->s.n, p->level->n_r, steps, p->level->B);
  return ZFFT_OK;
}

int zfft_level_push_device(zfft_plan *p, const void *d_x, int64_t steps, int64_t step_stride, const void *d_key,
                           int64_t key_stride, void *d_out, void *stream) {
  int rc = enter(p);
  if (!rc) rc = need_on(p);
  if (rc || steps == 0) return rc;
  rc = check_push(p->level, steps, step_stride, d_key != nullptr, key_stride);
  return rc ? rc : push_on(p, d_x, steps, step_stride, d_key, key_stride, d_out, stream);
}

int zfft_level_push(zfft_plan *p, const void *x, const void *key, int64_t steps, int64_t step_stride, void *out,
                    int64_t *outputs_out) {
  int rc = enter(p);
  if (!rc) rc = need_on(p);
  if (rc) return rc;
  int64_t outs = 0;
  rc = zfft_level_steps(p, steps, &outs);
  if (rc) return rc;
  if (outputs_out) *outputs_out = outs;
  if (steps == 0) return ZFFT_OK;
  LevelState *r = p->level;
  rc = check_push(r, steps, step_stride, false, 0);
  if (rc) return rc;
  if (!x) return fail(ZFFT_EINVAL, "level push: null host pointer");
  // the samples and, behind them at a 16-byte boundary, the key: one staged array
  const size_t count = (size_t)(steps - 1) * (size_t)step_stride + (size_t)r->K;
  const size_t key_at = (count + 3) & ~(size_t)3;
  const void *in = x;
  std::vector<float> both;
  if (key) {
    both.resize(key_at + count);
    std::copy((const float *)x, (const float *)x + count, both.begin());
    std::copy((const float *)key, (const float *)key + count, both.begin() + (ptrdiff_t)key_at);
    in = both.data();
  }
  const size_t floats = key ? key_at + count : count;
  return stream_host_push(p, r->s, kNames, in, floats * sizeof(float), out, (size_t)outs * (size_t)r->K * sizeof(float),
                          [=](const void *d_in, void *d_out) {
                            const void *d_key = key ? (const void *)((const float *)d_in + key_at) : nullptr;
                            return push_on(p, d_in, steps, step_stride, d_key, step_stride, d_out, p->stream);
                          });
}

int zfft_level_state(zfft_plan *p, uint64_t *steps_seen) {
  if (!p || !steps_seen) return fail(ZFFT_EINVAL, "null argument");
  int rc = need_on(p);
  if (!rc) *steps_seen = p->level->s.n;
  return rc;
}

int zfft_level_reset(zfft_plan *p, int64_t n0) {
  int rc = enter(p);
  if (!rc) rc = need_on(p);
  if (rc) return rc;
  rc = stream_reset(p, p->level->s, kNames, n0);
  if (!rc) p->level->n_r = (uint64_t)n0;
  return rc;
}

int zfft_level_info(const zfft_plan *p, double *latency_min, double *latency_max, double *rate_ratio) {
  if (!p || !latency_min || !latency_max || !rate_ratio) return fail(ZFFT_EINVAL, "null argument");
  int rc = need_on(p);
  if (rc) return rc;
  *latency_min = p->level->B;
  *latency_max = 2.0 * p->level->B - 1.0;
  *rate_ratio = 1.0;
  return ZFFT_OK;
}

int zfft_level_meter(zfft_plan *p, float *env_out, float *gain_out) {
  int rc = enter(p);
  if (!rc) rc = need_on(p);
  if (rc) return rc;
  if (!env_out || !gain_out) return fail(ZFFT_EINVAL, "null argument");
  LevelState *r = p->level;
  // the carried peaks end at the newest complete block: its envelope is the max of the last H + 1
  const size_t K = (size_t)r->K, rows = (size_t)r->H + 1;
  std::vector<float> tail(rows * K);
  rc = use_stream(p, p->stream);
  if (rc) return rc;
  const float *d_tail = (const float *)r->s.carry_in() + (size_t)(2 * r->B) * K + K;  // (row 1 of the H + 2)
  hipError_t e = hipMemcpyAsync(tail.data(), d_tail, tail.size() * sizeof(float), hipMemcpyDeviceToHost, p->stream);
  rc = sync_read(p, e, "level meter");
  if (rc) return rc;
  for (size_t s = 0; s < K; ++s) {
    float E = 0.f;
    for (size_t j = 0; j < rows; ++j) E = std::max(E, tail[j * K + s]);
    env_out[s] = E;
    gain_out[s] = level_gain(E, r->par[0], r->par[1], r->par[2], r->par[3]);
  }
  return ZFFT_OK;
}

}  // extern "C"
