// zfft_plan.cpp -- the plan of libzfft.so: create / destroy, its settings, the stream ordering
// helpers, the buffer and staging helpers of the row consumers (grow, sync_read, stage_rows,
// pin_rows) and the host entry points (zfft_process, zfft_decimate).  The plan object is in
// zfft_plan.h, the decimator in zfft_decim.cpp (schedule choice: zfft_schedule.cpp), the Welch
// launches in zfft_welch.cpp (form choice: zfft_welch_plan.cpp), the waterfall in
// zfft_waterfall.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "cheby1_q2.h"
#include "zfft.h"
#include "zfft_plan.h"
#include "zfft_schedule.h"
#include "zfft_welch_plan.h"

namespace zfft {

static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }

Sos32 sos32() {
  static const Sos32 c = [] {
    Sos32 s{};
    s.b0 = (float)kDecimSos[0][0];
    s.b1 = (float)kDecimSos[0][1];
    s.b2 = (float)kDecimSos[0][2];
    for (int k = 0; k < 4; ++k) {
      s.a1[k] = (float)kDecimSos[k][4];
      s.a2[k] = (float)kDecimSos[k][5];
      s.zi[k][0] = (float)kDecimZi[k][0];
      s.zi[k][1] = (float)kDecimZi[k][1];
    }
    return s;
  }();
  return c;
}

int fail(int code, const std::string &msg) {
  set_error(msg);
  return code;
}

int hip_fail(hipError_t e, const char *where) {
  return fail(ZFFT_EHIP, std::string(where) + ": " + hipGetErrorString(e));
}

void mark(zfft_plan *p, hipStream_t st, const char *what) {
  if (!p->timing) return;
  if ((int)p->events.size() <= p->n_marks) {
    hipEvent_t ev;
    if (hipEventCreate(&ev) != hipSuccess) return;
    p->events.push_back(ev);
  }
  if ((int)p->mark_names.size() <= p->n_marks) p->mark_names.resize(p->n_marks + 1);
  p->mark_names[p->n_marks] = what;
  (void)hipEventRecord(p->events[p->n_marks++], st);
}

int use_stream(zfft_plan *p, hipStream_t st) {
  if (p->has_work && p->done_st != st) {
    hipError_t e = hipStreamWaitEvent(st, p->done_ev, 0);
    if (e != hipSuccess) return hip_fail(e, "hipStreamWaitEvent");
  }
  return ZFFT_OK;
}
int begin_call(zfft_plan *p, void *hip_stream, hipStream_t *st) {
  *st = pick_stream(p, hip_stream);
  int rc = use_stream(p, *st);
  if (rc) return rc;
  p->n_marks = 0;
  mark(p, *st, "start");
  return ZFFT_OK;
}
int done_on(zfft_plan *p, hipStream_t st) {
  hipError_t e = hipEventRecord(p->done_ev, st);
  if (e != hipSuccess) return hip_fail(e, "hipEventRecord");
  p->done_st = st;
  p->has_work = true;
  return ZFFT_OK;
}
int quiesce(zfft_plan *p) {
  if (!p->has_work) return ZFFT_OK;
  ++p->n_quiesce;
  hipError_t e = hipEventSynchronize(p->done_ev);
  return e == hipSuccess ? ZFFT_OK : hip_fail(e, "hipEventSynchronize");
}

int grow(zfft_plan *p, DevBuf &b, size_t bytes, const char *what) {
  if (b.cap >= bytes) return ZFFT_OK;
  int rc = quiesce(p);  // growing frees what an enqueued call may still use
  if (rc) return rc;
  if (b.ensure(bytes) != hipSuccess) {
    (void)hipGetLastError();
    return fail(ZFFT_ENOMEM, std::string(what) + " allocation failed");
  }
  return ZFFT_OK;
}

int sync_read(zfft_plan *p, hipError_t e, const char *what) {
  if (e == hipSuccess) e = done_on(p, p->stream) == ZFFT_OK ? hipSuccess : hipErrorUnknown;
  if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
  return e == hipSuccess ? ZFFT_OK : hip_fail(e, what);
}

int stage_rows(zfft_plan *p, const float *rows, int32_t count, const char *what, const float **d_rows) {
  const size_t bytes = (size_t)count * p->cfg.n_win * sizeof(float);
  int rc = grow(p, p->row_stage, bytes, what);
  if (rc) return rc;
  rc = use_stream(p, p->stream);  // the staging may still be read by the previous call
  if (rc) return rc;
  hipError_t e = hipMemcpyAsync(p->row_stage.p, rows, bytes, hipMemcpyHostToDevice, p->stream);
  if (e != hipSuccess) return hip_fail(e, "H2D rows");
  *d_rows = p->row_stage.as<float>();
  return ZFFT_OK;
}

int pin_rows(zfft_plan *p, const float *rows, size_t bytes, const float **d_rows) {
  if (bytes > p->row_pin_cap) {
    int rc = quiesce(p);
    if (rc) return rc;
    if (p->row_pin) (void)hipHostFree(p->row_pin);
    p->row_pin = nullptr;
    p->row_pin_cap = 0;
    if (hipHostMalloc((void **)&p->row_pin, bytes, hipHostMallocDefault) != hipSuccess)
      return fail(ZFFT_ENOMEM, "page-locked row staging allocation failed");
    p->row_pin_cap = bytes;
  }
  std::memcpy(p->row_pin, rows, bytes);
  void *d = nullptr;
  hipError_t e = hipHostGetDevicePointer(&d, p->row_pin, 0);
  if (e != hipSuccess) return hip_fail(e, "hipHostGetDevicePointer");
  *d_rows = (const float *)d;
  return ZFFT_OK;
}

int enter(zfft_plan *p) {
  if (!p) return fail(ZFFT_EINVAL, "null plan");
  hipError_t e = hipSetDevice(p->cfg.device);
  if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
  return ZFFT_OK;
}

// The length of the reference's slice fftshift(P)[N//2 - W//2 : N//2 + W//2] (S:2114):
// 2 (W//2), or in the one-sided case that slice of the N/2+1 bins.
int row_length(const zfft_plan *p) {
  const int N = p->cfg.n_fft, W = p->cfg.n_win;
  if (!onesided(p)) return W & ~1;  // [N/2 - W//2, N/2 + W//2): W - 1 entries for odd W
  const int a = N / 2 - W / 2, b = std::min(N / 2 + W / 2, N / 2 + 1);
  return std::max(0, b - a);
}

int64_t lines_per_frame(const zfft_plan *p, int64_t L) {
  const int64_t r = zfft_line_count(L, p->cfg.zoom, p->cfg.n_fft, p->seg_per_line);
  return r < 1 ? 1 : r;  // (bad lengths are refused by the call itself)
}

}  // namespace zfft

using namespace zfft;

namespace {

bool is_pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }
int ilog2(int64_t v) {
  int r = 0;
  while ((int64_t(1) << r) < v) ++r;
  return r;
}

int check_lengths(const zfft_plan *p, int64_t L, int32_t frames, std::vector<int64_t> &n) {
  if (L < 1 || frames < 1) return fail(ZFFT_EINVAL, "n_samples and n_frames must be >= 1");
  if (L > (int64_t)1 << 30) return fail(ZFFT_EINVAL, "n_samples too large (max 2^30)");
  n = stage_lengths(L, p->K);
  for (int k = 0; k < p->K; ++k)
    if (n[k] <= kPad)
      return fail(ZFFT_ESHORT, "The length of the input vector x must be greater than padlen, "
                               "which is 27 (decimation stage " + std::to_string(k) + " has " +
                               std::to_string(n[k]) + " samples)");
  return ZFFT_OK;
}

constexpr int kMaxLoRows = 256;  // LO rows of set_lo_frames (each n_samples x 8 B)
// zfft_process pipelining: inputs of >= 64 MB go in batches of about 1 GB (at least two).
constexpr size_t kPipeMinBytes = (size_t)64 << 20;
constexpr size_t kPipeBatchBytes = (size_t)1 << 30;

InDesc input_of(const zfft_plan *p, const void *d_iq, int64_t L) {
  InDesc d{d_iq, L, L, p->cfg.in_dtype, p->cfg.flip_input};
  if (p->lo_freqs.size() > 1) {
    d.lo_stride = p->lo_len;  // (ensure_lo runs before any kernel reads the rows)
    d.lo_n = (int)p->lo_freqs.size();
    d.lo_per = p->lo_per;
    d.lo_first = p->lo_first;
  }
  return d;
}

int process_device(zfft_plan *p, const void *d_iq, int64_t L, int32_t frames, float *d_rows,
                   hipStream_t st) {
  std::vector<int64_t> n;
  int rc = check_lengths(p, L, frames, n);
  if (rc) return rc;
  const int64_t Ld = n[p->K];
  if (p->K > 0) {  // the LO rows exist (and have their stride) before input_of reads it
    rc = ensure_lo(p, L);
    if (rc) return rc;
  }
  const InDesc in = input_of(p, d_iq, L);
  const float2 *x = (const float2 *)d_iq;
  if (p->n_marks == 0) mark(p, st, "start");  // (the entry points reset the marks per call)
  if (p->K > 0) {
    rc = run_decimator(p, in, L, frames, n, &x, st);
    if (rc) return rc;
  } else if (in.dtype != kInC64 || in.flip) {  // zoom 1: Welch reads complex64 frames
    hipError_t e = p->dec.ensure((size_t)frames * L * sizeof(float2));
    if (e != hipSuccess) return fail(ZFFT_ENOMEM, "ingest workspace allocation failed");
    e = launch_ingest(in, nullptr, p->dec.as<float2>(), frames, st);
    if (e != hipSuccess) return hip_fail(e, "ingest launch");
    mark(p, st, "ingest");
    x = p->dec.as<float2>();
  }
  rc = run_welch(p, x, Ld, frames, d_rows, st);
  if (rc) return rc;
  p->last_row = d_rows + ((int64_t)frames * lines_per_frame(p, L) - 1) * p->cfg.n_win;
  return ZFFT_OK;
}

}  // namespace

// Test hook (not part of include/zfft.h): how often the plan has waited on the host for its
// enqueued work (a table upload that must not overwrite data in use, a synchronous call).
extern "C" int64_t zfft__plan_quiesce_count(const zfft_plan *p) { return p ? p->n_quiesce : -1; }

// Test hooks (not part of include/zfft.h): the cap of the median / max detectors' segment
// scratch in bytes (0 = the default), so that a small call runs in several chunks; and the
// number of workgroups per frame (WelchGeom::split) of the plan's last one-workgroup Welch launch.
extern "C" int zfft__plan_average_cap(zfft_plan *p, int64_t bytes) {
  if (!p || bytes < 0) return ZFFT_EINVAL;
  p->avg_cap = (size_t)bytes;
  return ZFFT_OK;
}
// Test / measurement hook: how mean lines run -- 0 the plan's choice (fused where a fused form
// exists), 1 the segment scratch route everywhere.
extern "C" int zfft__plan_lines_route(zfft_plan *p, int route) {
  if (!p || route < 0 || route > 1) return ZFFT_EINVAL;
  p->lines_route = route;
  return ZFFT_OK;
}
extern "C" int zfft__plan_welch_split(const zfft_plan *p) { return p ? p->last_split : -1; }

// Test hook (not part of include/zfft.h; needs no device): the decimator schedule a call of
// `frames` frames of L samples takes on a plan of this zoom, in_dtype and forced path --
// choose_schedule's rc, and schedule_name into name[cap].
extern "C" int zfft__schedule(int32_t zoom, int32_t in_dtype, int32_t path, int64_t L, int32_t frames,
                              char *name, int32_t cap) {
  if (!is_pow2(zoom) || in_dtype < kInC64 || in_dtype > kInF32R || !name || cap < 1) return ZFFT_EINVAL;
  const Schedule s = choose_schedule({ilog2(zoom), (int)in_elem_bytes(in_dtype), path, L, frames});
  std::snprintf(name, (size_t)cap, "%s", schedule_name(s));
  return s.rc;
}

// Test hook (not part of include/zfft.h; needs no device): the Welch form a call of `frames`
// frames of L samples takes on a plan of these settings -- choose_welch's rc, and one line naming
// everything that selects a kernel or a grid into desc[cap], e.g.
// "dif parts split=3 last_split=3 lines=1 chunk=2 select=none".
extern "C" int zfft__welch_plan(int32_t n_fft, int32_t n_win, int32_t zoom, int32_t in_dtype, int32_t welch,
                                int32_t average, int32_t seg_per_line, int32_t lines_route, int64_t cap_bytes,
                                int64_t L, int32_t frames, char *desc, int32_t cap) {
  if (!is_pow2(n_fft) || n_fft < 32 || n_fft > 65536 || n_win < 2 || n_win > n_fft || !is_pow2(zoom) ||
      zoom > 512 || in_dtype < kInC64 || in_dtype > kInF32R || average < ZFFT_AVG_MEAN || average > ZFFT_AVG_MAX ||
      seg_per_line < 0 || lines_route < 0 || lines_route > 1 || cap_bytes < 0 || L < 1 ||
      L > (int64_t)1 << 30 || frames < 1 || !desc || cap < 1)
    return ZFFT_EINVAL;
  const WelchPlan w = choose_welch({n_fft, n_win, zfft_decimated_length(L, zoom), frames,
                                    welch, average, seg_per_line, lines_route, (size_t)cap_bytes});
  if (w.rc)
    std::snprintf(desc, (size_t)cap, "refused");
  else
    std::snprintf(desc, (size_t)cap, "%s %s split=%d last_split=%d lines=%d chunk=%d select=%s", welch_fft_name(w.fft),
                  welch_out_name(w.out), w.split, w.split_last, w.lines, w.chunk, welch_sel_name(w.sel));
  return w.rc;
}

extern "C" {

const char *zfft_last_error(void) { return g_err.c_str(); }
int zfft_version(void) { return ZFFT_VERSION; }

int zfft_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int64_t zfft_decimated_length(int64_t n_samples, int32_t zoom) {
  if (n_samples < 0 || !is_pow2(zoom)) return -1;
  for (int z = zoom; z > 1; z >>= 1) n_samples = (n_samples + 1) / 2;
  return n_samples;
}

int zfft_plan_create(const zfft_config *cfg, const float *window_or_null, zfft_plan **out) {
  if (!cfg || !out) return fail(ZFFT_EINVAL, "null config or output pointer");
  *out = nullptr;
  const zfft_config &c = *cfg;
  if (!is_pow2(c.n_fft) || c.n_fft < 32 || c.n_fft > 65536)
    return fail(ZFFT_EINVAL, "n_fft must be a power of two in [32, 65536]");
  if (!is_pow2(c.zoom) || c.zoom > 512) return fail(ZFFT_EINVAL, "zoom must be 1, 2, 4, ..., 512");
  if (c.n_win < 2 || c.n_win > c.n_fft)
    return fail(ZFFT_EINVAL, "n_win must be in [2, n_fft]");
  if (!(c.fs > 0) || !std::isfinite(c.fs) || !std::isfinite(c.f_lo))
    return fail(ZFFT_EINVAL, "fs must be positive and finite, f_lo finite");
  if (c.scroll != 1 && c.scroll != -1) return fail(ZFFT_EINVAL, "scroll must be +1 or -1");
  if (c.in_dtype < kInC64 || c.in_dtype > kInF32R)
    return fail(ZFFT_EINVAL, "in_dtype must be 0 (complex64), 1 (complex32 f16), 2 (RTL-SDR u8) or 3 (real f32)");
  if (c.flip_input != 0 && c.flip_input != 1) return fail(ZFFT_EINVAL, "flip_input must be 0 or 1");
  if (c.window_kind == ZFFT_WIN_ARRAY) {
    if (!window_or_null) return fail(ZFFT_EINVAL, "ZFFT_WIN_ARRAY needs a window array");
  } else if (!window_kind_native(c.window_kind)) {
    return fail(ZFFT_EINVAL, "unknown window kind");
  }
  int ndev = zfft_device_count();
  if (ndev < 1) return fail(ZFFT_ENODEV, "no HIP device");
  if (c.device < 0 || c.device >= ndev) return fail(ZFFT_ENODEV, "device ordinal out of range");
  hipError_t e = hipSetDevice(c.device);
  if (e != hipSuccess) return hip_fail(e, "hipSetDevice");

  zfft_plan *p = new zfft_plan();
  p->cfg = c;
  p->K = ilog2(c.zoom);
  if (c.window_kind == ZFFT_WIN_ARRAY)
    p->user_window.assign(window_or_null, window_or_null + c.n_fft);
  e = hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&p->copy_st, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&p->done_ev, hipEventDisableTiming);
  for (int i = 0; i < 2 && e == hipSuccess; ++i) {
    e = hipEventCreateWithFlags(&p->h2d_ev[i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&p->comp_ev[i], hipEventDisableTiming);
  }
  if (e != hipSuccess) {
    zfft_plan_destroy(p);
    return hip_fail(e, "hipStreamCreate / hipEventCreate");
  }
  // FFT twiddles tw[m] = exp(-2 pi i m / N), computed in fp64
  std::vector<float2> tw(c.n_fft);
  for (int m = 0; m < c.n_fft; ++m) {
    const double a = -2.0 * M_PI * (double)m / (double)c.n_fft;
    tw[m] = make_float2((float)std::cos(a), (float)std::sin(a));
  }
  e = p->tw.ensure(c.n_fft * sizeof(float2));
  if (e == hipSuccess)
    e = hipMemcpy(p->tw.p, tw.data(), c.n_fft * sizeof(float2), hipMemcpyHostToDevice);
  if (e == hipSuccess && c.n_fft >= 4096) {  // four-step sub-FFT twiddles: W_256 ++ W_N1
    const int n1 = c.n_fft / 256;
    std::vector<float2> ts(256 + n1);
    for (int m = 0; m < 256; ++m) ts[m] = tw[(size_t)m * n1];
    for (int m = 0; m < n1; ++m) ts[256 + m] = tw[(size_t)m * 256];
    e = p->tws.ensure(ts.size() * sizeof(float2));
    if (e == hipSuccess)
      e = hipMemcpy(p->tws.p, ts.data(), ts.size() * sizeof(float2), hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) {
    static XaTab xa[1]{};
    static const bool xa_ok = xa_build_tables(xa[0], kXaB);
    if (!xa_ok) {
      zfft_plan_destroy(p);
      return fail(ZFFT_EHIP, "XA tables: scan levels too shallow for the filter poles");
    }
    e = p->xa_tab.ensure(sizeof(xa));
    if (e == hipSuccess) e = hipMemcpy(p->xa_tab.p, xa, sizeof(xa), hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    zfft_plan_destroy(p);
    return hip_fail(e, "twiddle upload");
  }
  *out = p;
  return ZFFT_OK;
}

int zfft_plan_destroy(zfft_plan *p) {
  if (!p) return ZFFT_OK;
  (void)hipSetDevice(p->cfg.device);
  // every stream idle before anything it may still use goes away
  if (p->has_work) (void)hipEventSynchronize(p->done_ev);
  for (hipStream_t s : {p->stream, p->copy_st})
    if (s) (void)hipStreamSynchronize(s);
  if (p->row_pin) (void)hipHostFree(p->row_pin);
  tap_release(p);  // (its page-locked staging)
  chan_release(p);
  demod_release(p);
  resamp_release(p);
  level_release(p);
  for (hipEvent_t ev : p->events) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : {p->done_ev, p->h2d_ev[0], p->h2d_ev[1], p->comp_ev[0], p->comp_ev[1]})
    if (ev) (void)hipEventDestroy(ev);
  for (hipStream_t s : {p->stream, p->copy_st})
    if (s) (void)hipStreamDestroy(s);
  delete p;  // frees the device buffers (DevBuf)
  return ZFFT_OK;
}

int zfft_plan_row_length(const zfft_plan *p) {
  if (!p) return fail(ZFFT_EINVAL, "null plan");
  return row_length(p);
}

int zfft_plan_config(const zfft_plan *p, zfft_config *out) {
  if (!p || !out) return fail(ZFFT_EINVAL, "null argument");
  *out = p->cfg;
  return ZFFT_OK;
}

int zfft_plan_tune(zfft_plan *p, int32_t block, int32_t warm) {
  if (!p || block < 0 || warm < 0) return fail(ZFFT_EINVAL, "bad tune arguments");
  if (block && (block < 64 || block > (1 << 20)))
    return fail(ZFFT_EINVAL, "block must be in [64, 2^20]");
  p->block_override = block;
  p->warm_override = warm;
  return ZFFT_OK;
}

int zfft_plan_timing(zfft_plan *p, int32_t enable) {
  if (!p) return fail(ZFFT_EINVAL, "null plan");
  p->timing = enable != 0;  // marks of the last timed call stay readable
  return ZFFT_OK;
}

int zfft_plan_path(zfft_plan *p, int32_t path) {
  if (!p || path < 0 || path > 7)
    return fail(ZFFT_EINVAL, "path must be 0 (auto), 1 (exact), 2 (fused), 3 (XA tiles), 4 (PC "
                             "tiles), 5 (PC walk), 6 (FC at zoom 8 and 4, else as 5) or 7 (FC at "
                             "zoom 2 and for the tails of zoom >= 16 too, else as 6)");
  p->path = path;
  return ZFFT_OK;
}

int zfft_plan_set_lo_frames(zfft_plan *p, const double *f_lo, int32_t n, int32_t frames_per_lo) {
  int rc = enter(p);
  if (rc) return rc;
  if (n < 0 || n > kMaxLoRows || (n > 0 && (!f_lo || frames_per_lo < 1)))
    return fail(ZFFT_EINVAL, "set_lo_frames: 0 <= n <= 256 frequencies, frames_per_lo >= 1");
  if (n > 1 && p->K == 0)  // rows never mix at zoom 1: the reference skips zoomfft (S:2108)
    return fail(ZFFT_EINVAL, "set_lo_frames: several LO rows need zoom > 1 (zoom 1 does not mix)");
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(f_lo[i])) return fail(ZFFT_EINVAL, "set_lo_frames: f_lo must be finite");
  rc = quiesce(p);  // the old table may still be read by enqueued work
  if (rc) return rc;
  p->lo_freqs.assign(f_lo, f_lo + n);
  if (n == 1) p->cfg.f_lo = f_lo[0];
  if (n <= 1) p->lo_freqs.clear();
  p->lo_per = n > 0 ? frames_per_lo : 1;
  p->lo_len = 0;  // rebuilt by the next call
  return ZFFT_OK;
}

int zfft_plan_welch(zfft_plan *p, int32_t mode) {
  if (!p) return fail(ZFFT_EINVAL, "null plan");
  const char *why;
  const int rc = welch_mode_rc(p->cfg.n_fft, mode, &why);
  if (rc) return fail(rc, why);
  p->welch = mode;
  return ZFFT_OK;
}

int zfft_plan_segments_per_line(zfft_plan *p, int32_t g) {
  if (!p) return fail(ZFFT_EINVAL, "null plan");
  if (g < 0) return fail(ZFFT_EINVAL, "segments_per_line must be 0 (the whole frame) or >= 1");
  p->seg_per_line = g;
  return ZFFT_OK;
}

int64_t zfft_line_count(int64_t n_samples, int32_t zoom, int32_t n_fft, int32_t g) {
  if (n_samples < 1 || n_fft < 2 || g < 0) return -1;
  const int64_t Ld = zfft_decimated_length(n_samples, zoom);
  if (Ld < 1) return -1;
  return welch_segments(Ld, n_fft, g).lines;  // (short input: one segment of L_d samples, one line)
}

int zfft_line_times(int64_t n_samples, int32_t zoom, int32_t n_fft, double fs, int32_t g, double *t_out,
                    int32_t max, int32_t *count) {
  if (!t_out || !count) return fail(ZFFT_EINVAL, "line_times: null output");
  *count = 0;
  const int64_t R = zfft_line_count(n_samples, zoom, n_fft, g);
  if (R < 1 || !(fs > 0) || !std::isfinite(fs))
    return fail(ZFFT_EINVAL, "line_times: n_samples >= 1, zoom a power of two, n_fft >= 2, fs > 0, "
                             "segments_per_line >= 0");
  if (R > INT32_MAX) return fail(ZFFT_EINVAL, "line_times: too many lines");
  *count = (int32_t)R;
  if (max < R) return fail(ZFFT_EINVAL, "line_times: max is smaller than zfft_line_count");
  const WelchSegments s = welch_segments(zfft_decimated_length(n_samples, zoom), n_fft, g);
  for (int64_t r = 0; r < R; ++r) {
    // the mean of t_s over line r's n segments from s0: its middle segment (a half step when n is even)
    const int64_t s0 = r * s.grp, n = r < R - 1 ? s.grp : s.tail;
    const double mid = (double)s0 + 0.5 * (double)(n - 1);
    t_out[r] = (mid * (double)s.step + 0.5 * (double)s.nperseg) * (double)zoom / fs;
  }
  return ZFFT_OK;
}

int zfft_plan_average(zfft_plan *p, int32_t mode) {
  if (!p) return fail(ZFFT_EINVAL, "null plan");
  if (mode != ZFFT_AVG_MEAN && mode != ZFFT_AVG_MEDIAN && mode != ZFFT_AVG_MAX)
    return fail(ZFFT_EINVAL, "average must be 0 (mean), 1 (median) or 2 (max)");
  p->average = mode;
  return ZFFT_OK;
}

const char *zfft_plan_timing_names(zfft_plan *p) {
  if (!p) return "";
  p->names_buf.clear();
  for (int k = 1; k < p->n_marks; ++k) {
    if (k > 1) p->names_buf += ",";
    p->names_buf += p->mark_names[k];
  }
  return p->names_buf.c_str();
}

int zfft_plan_timings(zfft_plan *p, float *ms_out, int32_t max, int32_t *count) {
  int rc = enter(p);
  if (rc) return rc;
  if (!ms_out || !count) return fail(ZFFT_EINVAL, "null output");
  const int n = p->n_marks > 0 ? p->n_marks - 1 : 0;
  if (n > 0) {
    hipError_t e = hipEventSynchronize(p->events[n]);
    if (e != hipSuccess) return hip_fail(e, "event sync");
  }
  int k = 0;
  for (; k < n && k < max; ++k) {
    float ms = 0.f;
    hipError_t e = hipEventElapsedTime(&ms, p->events[k], p->events[k + 1]);
    if (e != hipSuccess) return hip_fail(e, "event elapsed");
    ms_out[k] = ms;
  }
  *count = k;
  return ZFFT_OK;
}

int zfft_process_device(zfft_plan *p, const void *d_iq, int64_t L, int32_t frames, float *d_rows,
                        void *hip_stream) {
  int rc = enter(p);
  if (rc) return rc;
  if (!d_iq || !d_rows) return fail(ZFFT_EINVAL, "null device pointer");
  hipStream_t st = pick_stream(p, hip_stream);
  rc = use_stream(p, st);
  if (rc) return rc;
  p->n_marks = 0;
  rc = process_device(p, d_iq, L, frames, d_rows, st);
  if (rc) return rc;
  return done_on(p, st);
}

int zfft_process(zfft_plan *p, const void *iq, int64_t L, int32_t frames, float *rows_out) {
  int rc = enter(p);
  if (rc) return rc;
  if (!iq || !rows_out) return fail(ZFFT_EINVAL, "null host pointer");
  if (L < 1 || frames < 1) return fail(ZFFT_EINVAL, "n_samples and n_frames must be >= 1");
  const size_t frame_bytes = (size_t)L * in_elem_bytes(p->cfg.in_dtype);
  // rows per frame (zfft_plan_segments_per_line): every row-sized quantity below scales by it
  const int64_t R = lines_per_frame(p, L);
  const size_t row_bytes = (size_t)frames * (size_t)R * p->cfg.n_win * sizeof(float);
  // Batches: one for a small call; otherwise >= 2 so that the H2D copy of batch k+1 (copy
  // stream) runs while batch k is computed (plan stream).  From pinned memory both are
  // asynchronous; from pageable memory HIP stages the copy on this thread, which then copies
  // batch k+1 while the GPU computes batch k.  Every batch takes the schedule its own frame
  // count earns (choose_schedule, per batch).  A call that XA would take -- all stages, or the
  // stages after the PC / FC head of zoom >= 16 -- keeps XA in every batch: its batches hold
  // at least the XA threshold for this frame length (or the call is one batch), so splitting
  // never drops a large call onto a schedule that loses at its batch size.  Where PC or FC
  // takes the whole call (zoom 8 and 4, zoom 2 below 512 frames) no such floor is needed: they
  // win at every batch (e.g. cfg2's 418-frame batches run FC, a 12-frame batch zoom 8's tiles).
  int B = frames;
  const size_t total = (size_t)frames * frame_bytes;
  if (total >= kPipeMinBytes && frames >= 2) {
    int nb = std::max<int64_t>(2, (int64_t)((total + kPipeBatchBytes - 1) / kPipeBatchBytes));
    B = (frames + nb - 1) / nb;
    const int need = xa_min_frames(L);
    if (B < need && batches_keep_xa({p->K, (int)in_elem_bytes(p->cfg.in_dtype), p->path, L, frames})) {
      nb = std::max(1, frames / need);
      B = (frames + nb - 1) / nb;
    }
  }
  const int nb = (frames + B - 1) / B;
  hipError_t e = p->in.ensure((size_t)B * frame_bytes);
  if (e == hipSuccess && nb > 1) e = p->in2.ensure((size_t)B * frame_bytes);
  if (e == hipSuccess) e = p->rows.ensure(row_bytes);
  if (e != hipSuccess) return fail(ZFFT_ENOMEM, "staging allocation failed");
  rc = use_stream(p, p->stream);
  if (rc == ZFFT_OK && nb > 1) rc = use_stream(p, p->copy_st);
  if (rc) return rc;
  const char *src = (const char *)iq;
  p->n_marks = 0;  // timings cover every batch of this call
  mark(p, p->stream, "start");
  for (int k = 0; k < nb; ++k) {
    const int f0 = k * B, nk = std::min(B, frames - f0), buf = k & 1;
    void *dst = buf ? p->in2.p : p->in.p;
    hipStream_t cs = nb > 1 ? p->copy_st : p->stream;
    if (k >= 2) e = hipStreamWaitEvent(cs, p->comp_ev[buf], 0);  // batch k-2 done with dst
    if (e == hipSuccess) e = hipMemcpyAsync(dst, src + (size_t)f0 * frame_bytes, (size_t)nk * frame_bytes,
                                            hipMemcpyHostToDevice, cs);
    if (e == hipSuccess && nb > 1) e = hipEventRecord(p->h2d_ev[buf], cs);
    if (e == hipSuccess && nb > 1) e = hipStreamWaitEvent(p->stream, p->h2d_ev[buf], 0);
    if (e != hipSuccess) return hip_fail(e, "H2D copy");
    if (k > 0) mark(p, p->stream, "batch_wait");
    p->lo_first = f0;  // batch frame 0 is call frame f0 (its LO row, config 4)
    rc = process_device(p, dst, L, nk, p->rows.as<float>() + (int64_t)f0 * R * p->cfg.n_win, p->stream);
    p->lo_first = 0;
    if (rc) return rc;
    if (nb > 1 && (e = hipEventRecord(p->comp_ev[buf], p->stream)) != hipSuccess)
      return hip_fail(e, "event record");
  }
  e = hipMemcpyAsync(rows_out, p->rows.p, row_bytes, hipMemcpyDeviceToHost, p->stream);
  if (e != hipSuccess) return hip_fail(e, "D2H copy");
  rc = done_on(p, p->stream);
  if (rc) return rc;
  e = hipStreamSynchronize(p->stream);
  return e == hipSuccess ? ZFFT_OK : hip_fail(e, "sync");
}

int zfft_decimate(zfft_plan *p, const void *iq, int64_t L, void *out_iq, int64_t *out_len) {
  return zfft_decimate_frames(p, iq, L, 1, out_iq, out_len);
}

int zfft_decimate_frames(zfft_plan *p, const void *iq, int64_t L, int32_t frames, void *out_iq,
                         int64_t *out_len) {
  int rc = enter(p);
  if (rc) return rc;
  if (!iq || !out_iq) return fail(ZFFT_EINVAL, "null host pointer");
  std::vector<int64_t> n;
  rc = check_lengths(p, L, frames, n);
  if (rc) return rc;
  const size_t in_bytes = (size_t)frames * L * in_elem_bytes(p->cfg.in_dtype);
  rc = ensure_lo(p, L);  // (a table upload waits for the plan's earlier work)
  if (rc) return rc;
  hipError_t e = p->in.ensure(in_bytes);
  if (e != hipSuccess) return fail(ZFFT_ENOMEM, "staging allocation failed");
  rc = use_stream(p, p->stream);
  if (rc) return rc;
  e = hipMemcpyAsync(p->in.p, iq, in_bytes, hipMemcpyHostToDevice, p->stream);
  if (e != hipSuccess) return hip_fail(e, "H2D copy");
  p->n_marks = 0;  // timings of this call's launches (the first one was unnamed before)
  mark(p, p->stream, "start");
  const float2 *x;
  if (p->K == 0) {  // zoomfft(x, 1) still mixes (S:2093-2094)
    e = p->dec.ensure((size_t)frames * L * sizeof(float2));
    if (e != hipSuccess) return fail(ZFFT_ENOMEM, "allocation failed");
    e = launch_ingest(input_of(p, p->in.p, L), p->lo.as<float2>(), p->dec.as<float2>(), frames,
                      p->stream);
    if (e != hipSuccess) return hip_fail(e, "mix launch");
    x = p->dec.as<float2>();
  } else {
    rc = run_decimator(p, input_of(p, p->in.p, L), L, frames, n, &x, p->stream);
    if (rc) return rc;
  }
  const int64_t m = n[p->K];
  e = hipMemcpyAsync(out_iq, x, (size_t)frames * m * sizeof(float2), hipMemcpyDeviceToHost, p->stream);
  if (e != hipSuccess) return hip_fail(e, "D2H copy");
  rc = done_on(p, p->stream);
  if (rc) return rc;
  e = hipStreamSynchronize(p->stream);
  if (e != hipSuccess) return hip_fail(e, "sync");
  if (out_len) *out_len = m;
  return ZFFT_OK;
}
}  // extern "C"
