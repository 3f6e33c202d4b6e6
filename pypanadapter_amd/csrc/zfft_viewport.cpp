// zfft_viewport.cpp -- the display viewport of libzfft.so: the rows the caller pushes reduced on
// the device to a ring of display-sized lines (a bucket of columns per pixel, rows_per_line rows
// per line, MAX / MIN / MEAN) and the traces last / max hold / min hold at that width (C-ABI and
// rule: zfft.h; kernels: view_kernels.hip; form chooser: zfft_view_plan.h).  The
// model is zfft_persist.cpp's: nothing runs inside zfft_process*.
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>

#include "zfft.h"
#include "zfft_plan.h"

using namespace zfft;

namespace {

const float kNaN = std::numeric_limits<float>::quiet_NaN();

int need_on(const zfft_plan *p) {
  return p->vw_h ? ZFFT_OK : fail(ZFFT_EINVAL, "the viewport is off (zfft_plan_viewport)");
}

size_t cells(const zfft_plan *p) { return (size_t)p->vw_h * p->vw_w; }

int fill(zfft_plan *p, float *dst, int64_t n) {
  hipError_t e = launch_view_fill(dst, n, kNaN, p->stream);
  return e == hipSuccess ? ZFFT_OK : hip_fail(e, "viewport fill");
}

// image, traces, pending group and counters as after the enable
int reset_view(zfft_plan *p) {
  int rc = use_stream(p, p->stream);
  if (rc) return rc;
  rc = fill(p, p->vw_ring.as<float>(), (int64_t)cells(p));
  if (!rc) rc = fill(p, p->vw_tr.as<float>(), 3 * (int64_t)p->vw_w);
  if (rc) return rc;
  p->vw_scroll = p->cfg.scroll;
  p->vw_off = 0;
  p->vw_rows = p->vw_lines = 0;
  p->vw_pending = 0;
  return done_on(p, p->stream);
}

void release_view(zfft_plan *p) {
  for (zfft_plan::DevBuf *b : {&p->vw_ring, &p->vw_img, &p->vw_tr, &p->vw_pend, &p->vw_scratch, &p->vw_rgba,
                               &p->row_stage})
    b->release();
  p->vw_h = p->vw_w = 0;
  p->vw_rows = p->vw_lines = 0;
  p->vw_pending = 0;
}

}  // namespace

// Test hook (not part of include/zfft.h): ViewForm::kind of the plan's last viewport push.
extern "C" int zfft__plan_view_form(const zfft_plan *p) { return p ? p->vw_kind : -1; }

extern "C" {

int zfft_plan_viewport(zfft_plan *p, int32_t height, int32_t width, int32_t col0, int32_t col1, int32_t detector,
                       int32_t rows_per_line) {
  int rc = enter(p);
  if (rc) return rc;
  rc = quiesce(p);  // an enqueued push may still use what is freed or replaced here
  if (rc) return rc;
  if (height == 0) {
    release_view(p);
    return ZFFT_OK;
  }
  const int n = row_length(p);
  if (col0 < 0 || col1 <= col0 || col1 > n || width < 1 || width > col1 - col0 || height < 1 ||
      height > kViewMaxHeight || (int64_t)height * width > kViewMaxPixels || rows_per_line < 1 ||
      rows_per_line > kViewMaxGroup || detector < ZFFT_VIEW_MAX || detector > ZFFT_VIEW_MEAN)
    return fail(ZFFT_EINVAL, "viewport: height 0 (off) or in [1, 8192], 0 <= col0 < col1 <= row length, 1 <= width "
                             "<= col1 - col0, height * width <= 2^25, rows_per_line in [1, 65536], detector 0..2");
  const size_t px = (size_t)height * width;
  if (p->vw_ring.ensure(px * sizeof(float)) != hipSuccess || p->vw_img.ensure(px * sizeof(float)) != hipSuccess ||
      p->vw_tr.ensure((size_t)3 * width * sizeof(float)) != hipSuccess ||
      p->vw_pend.ensure((size_t)width * sizeof(double)) != hipSuccess) {
    release_view(p);
    return fail(ZFFT_ENOMEM, "viewport allocation failed");
  }
  p->vw_h = height;
  p->vw_w = width;
  p->vw_c0 = col0;
  p->vw_c1 = col1;
  p->vw_det = detector;
  p->vw_m = rows_per_line;
  return reset_view(p);
}

int zfft_viewport_shape(const zfft_plan *p, int32_t *height, int32_t *width) {
  if (!p || !height || !width) return fail(ZFFT_EINVAL, "null argument");
  *height = p->vw_h;
  *width = p->vw_w;
  return need_on(p);
}

int zfft_viewport_push_device(zfft_plan *p, const float *d_rows, int32_t count, void *hip_stream) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  if (!d_rows || count < 1 || count > kMaxPushRows) return fail(ZFFT_EINVAL, "bad rows / count");
  ViewGeom g{};
  g.n_win = p->cfg.n_win;
  g.col0 = p->vw_c0;
  g.span = p->vw_c1 - p->vw_c0;
  g.width = p->vw_w;
  g.det = p->vw_det;
  g.m = p->vw_m;
  g.H = p->vw_h;
  g.off0 = (int)p->vw_off;
  g.scroll = p->vw_scroll;
  g.count = count;
  g.pending = p->vw_pending;
  const int64_t total = (int64_t)g.pending + count;
  g.ncomp = (int)(total / g.m);
  const ViewForm f = choose_view(count, g.m, g.pending, g.span, g.width);
  if (!f.ok()) return fail(ZFFT_EINTERNAL, "viewport: no form for this push");
  g.direct = view_direct(g, f) ? 1 : 0;
  rc = grow(p, p->vw_scratch, view_scratch_bytes(f, g.width), "viewport scratch");
  if (rc) return rc;
  hipStream_t st;
  rc = begin_call(p, hip_stream, &st);  // after the fills and earlier pushes, on any stream
  if (rc) return rc;
  hipError_t e = launch_view_lines(d_rows, g, f, p->vw_ring.as<float>(), p->vw_tr.as<float>(), p->vw_scratch.p,
                                   p->vw_scratch.cap, st);
  if (e != hipSuccess) return hip_fail(e, "viewport push");
  mark(p, st, "view_lines");
  if (!g.direct) {
    e = launch_view_finish(g, f, p->vw_ring.as<float>(), p->vw_tr.as<float>(), p->vw_pend.p, p->vw_scratch.p,
                           p->vw_scratch.cap, st);
    if (e != hipSuccess) return hip_fail(e, "viewport finish");
    mark(p, st, "view_finish");
  }
  p->vw_kind = f.kind;
  p->vw_rows += (uint64_t)count;
  p->vw_lines += (uint64_t)g.ncomp;
  p->vw_pending = (int)(total % g.m);
  p->vw_off = ((p->vw_off + (int64_t)g.ncomp * g.scroll) % g.H + g.H) % g.H;
  return done_on(p, st);
}

int zfft_viewport_push(zfft_plan *p, const float *rows, int32_t count) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  if (!rows || count < 1 || count > kMaxPushRows) return fail(ZFFT_EINVAL, "bad rows / count");
  const float *d_rows;
  rc = stage_rows(p, rows, count, "viewport row staging", &d_rows);
  if (!rc) rc = zfft_viewport_push_device(p, d_rows, count, p->stream);
  if (rc) return rc;
  hipError_t e = hipStreamSynchronize(p->stream);
  return e == hipSuccess ? ZFFT_OK : hip_fail(e, "sync");
}

int zfft_viewport_state(zfft_plan *p, uint64_t *rows_seen, uint64_t *lines, int32_t *pending) {
  if (!p) return fail(ZFFT_EINVAL, "null plan");
  int rc = need_on(p);
  if (rc) return rc;
  if (rows_seen) *rows_seen = p->vw_rows;
  if (lines) *lines = p->vw_lines;
  if (pending) *pending = p->vw_pending;
  return ZFFT_OK;
}

int zfft_viewport_read(zfft_plan *p, float *img_out) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  if (!img_out) return fail(ZFFT_EINVAL, "null output");
  rc = use_stream(p, p->stream);
  if (rc) return rc;
  hipError_t e = launch_waterfall_read(p->vw_ring.as<float>(), p->vw_h, p->vw_w, p->vw_off, p->vw_img.as<float>(),
                                       p->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(img_out, p->vw_img.p, cells(p) * sizeof(float), hipMemcpyDeviceToHost, p->stream);
  return sync_read(p, e, "viewport read");
}

int zfft_viewport_traces(zfft_plan *p, float *last, float *max_hold, float *min_hold) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  rc = use_stream(p, p->stream);
  if (rc) return rc;
  float *out[3] = {last, max_hold, min_hold};
  hipError_t e = hipSuccess;
  for (int k = 0; k < 3 && e == hipSuccess; ++k)
    if (out[k])
      e = hipMemcpyAsync(out[k], p->vw_tr.as<float>() + (size_t)k * p->vw_w, (size_t)p->vw_w * sizeof(float),
                         hipMemcpyDeviceToHost, p->stream);
  return sync_read(p, e, "viewport traces");
}

int zfft_viewport_hold_reset(zfft_plan *p) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  rc = use_stream(p, p->stream);
  if (rc) return rc;
  rc = fill(p, p->vw_tr.as<float>() + p->vw_w, 2 * (int64_t)p->vw_w);
  return rc ? rc : done_on(p, p->stream);
}

int zfft_viewport_reset(zfft_plan *p) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  return reset_view(p);
}

int zfft_viewport_render_device(zfft_plan *p, uint8_t *d_rgba, void *hip_stream) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  if (!d_rgba) return fail(ZFFT_EINVAL, "null output");
  hipStream_t st = pick_stream(p, hip_stream);
  rc = use_stream(p, st);
  if (rc) return rc;
  double lo, scale;
  rc = render_setup(p, st, &lo, &scale);
  if (rc) return rc;
  hipError_t e = launch_waterfall_render(p->vw_ring.as<float>(), p->vw_h, p->vw_w, p->vw_off, p->lut_d.p, lo, scale,
                                         d_rgba, st);
  if (e != hipSuccess) return hip_fail(e, "viewport render");
  return done_on(p, st);
}

int zfft_viewport_push_render(zfft_plan *p, const float *rows, int32_t count, uint8_t *rgba_out) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  if (!rgba_out) return fail(ZFFT_EINVAL, "null output");
  if (count < 0 || count > kMaxPushRows || (count > 0 && !rows)) return fail(ZFFT_EINVAL, "bad rows / count");
  const size_t bytes = cells(p) * 4;
  rc = grow(p, p->vw_rgba, bytes, "render buffer");  // (an enqueued render of the caller's never uses vw_rgba)
  if (rc) return rc;
  if (count > 0) {
    const float *d_rows;
    rc = pin_rows(p, rows, (size_t)count * p->cfg.n_win * sizeof(float), &d_rows);
    if (!rc) rc = zfft_viewport_push_device(p, d_rows, count, p->stream);
    if (rc) return rc;
  }
  // a small image into page-locked host memory is written by the kernel in place; a larger one
  // (1080 x 1920 is 8.3 MB) goes through the device buffer and one DMA copy
  void *dout = p->vw_rgba.p, *hout = nullptr;
  if (bytes <= kDisplayZeroCopyMax && hipHostGetDevicePointer(&hout, rgba_out, 0) == hipSuccess && hout)
    dout = hout;
  else
    (void)hipGetLastError(), hout = nullptr;
  rc = zfft_viewport_render_device(p, (uint8_t *)dout, p->stream);
  if (rc) return rc;
  hipError_t e = hout ? hipSuccess : hipMemcpyAsync(rgba_out, dout, bytes, hipMemcpyDeviceToHost, p->stream);
  return sync_read(p, e, "viewport image copy");
}

int zfft_viewport_render(zfft_plan *p, uint8_t *rgba_out) { return zfft_viewport_push_render(p, nullptr, 0, rgba_out); }

}  // extern "C"
