// zfft_history.cpp -- the row history of libzfft.so: the rows the caller pushes kept on the device
// as a ring of float32 rows or of 16- / 8-bit codes, read back, re-reduced to any window, time
// scale and detector, and replayed into the live viewport (C-ABI and rule: zfft.h; kernels:
// history_kernels.hip; quantiser and form chooser: zfft_history_plan.h).  The
// model is zfft_viewport.cpp's: nothing runs inside zfft_process*.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "zfft.h"
#include "zfft_plan.h"

using namespace zfft;

namespace {

constexpr size_t kReplayChunk = (size_t)64 << 20;    // float rows per replay step, bytes
const float kNaN = std::numeric_limits<float>::quiet_NaN();

int need_on(const zfft_plan *p) {
  return p->hs_cap ? ZFFT_OK : fail(ZFFT_EINVAL, "the row history is off (zfft_plan_history)");
}

void release_history(zfft_plan *p) {
  for (zfft_plan::DevBuf *b : {&p->hs_store, &p->row_stage, &p->hs_img, &p->hs_rgba, &p->hs_scratch, &p->hs_replay})
    b->release();
  p->hs_cap = p->hs_stride = 0;
  p->hs_seen = 0;
  p->hs_q = HistQuant();
}

HistStore store_of(const zfft_plan *p) {
  return HistStore{p->hs_store.p, p->hs_cap, p->hs_stride, row_length(p), p->hs_q};
}

uint64_t oldest_of(const zfft_plan *p) { return p->hs_seen - std::min<uint64_t>(p->hs_seen, (uint64_t)p->hs_cap); }

int window_ok(const zfft_plan *p, const zfft_history_window *w) {
  const int n = row_length(p);
  if (!w || w->col0 < 0 || w->col1 <= w->col0 || w->col1 > n || w->width < 1 || w->width > w->col1 - w->col0 ||
      w->lines < 1 || w->lines > kViewMaxHeight || (int64_t)w->lines * w->width > kViewMaxPixels ||
      w->rows_per_line < 1 || w->rows_per_line > kViewMaxGroup || w->detector < ZFFT_VIEW_MAX ||
      w->detector > ZFFT_VIEW_MEAN)
    return fail(ZFFT_EINVAL, "history window: 0 <= col0 < col1 <= row length, 1 <= width <= col1 - col0, lines in "
                             "[1, 8192], lines * width <= 2^25, rows_per_line in [1, 65536], detector 0..2");
  // (first + lines * rows_per_line stays far inside int64)
  if (w->first < -((int64_t)1 << 62) || w->first > ((int64_t)1 << 62)) return fail(ZFFT_EINVAL, "history window: first");
  return ZFFT_OK;
}

}  // namespace

// Test hook (not part of include/zfft.h): HistForm::kind of the plan's last view.
extern "C" int zfft__plan_history_form(const zfft_plan *p) { return p ? p->hs_kind : -1; }

extern "C" {

int zfft_plan_history(zfft_plan *p, int64_t capacity_rows, int32_t format, double db_min, double db_max) {
  int rc = enter(p);
  if (rc) return rc;
  rc = quiesce(p);  // an enqueued push or view may still use what is freed or replaced here
  if (rc) return rc;
  if (capacity_rows == 0) {
    release_history(p);
    return ZFFT_OK;
  }
  HistQuant q;
  const int n = row_length(p);
  if (capacity_rows < 1 || n < 1 || !hist_quant(format, db_min, db_max, &q))
    return fail(ZFFT_EINVAL, "history: capacity_rows 0 (off) or >= 1, format 0..2 and, for the coded formats, "
                             "finite db_min < db_max");
  const int64_t stride = hist_stride(n);
  const int64_t eb = hist_elem_bytes(format);
  release_history(p);  // re-enabling resets; a smaller store gives its memory back
  if (capacity_rows > std::numeric_limits<int64_t>::max() / (stride * eb) ||
      p->hs_store.ensure((size_t)capacity_rows * stride * eb) != hipSuccess) {
    (void)hipGetLastError();
    release_history(p);
    return fail(ZFFT_ENOMEM, "history store allocation failed");
  }
  p->hs_cap = capacity_rows;
  p->hs_stride = stride;
  p->hs_q = q;
  p->hs_seen = 0;
  return ZFFT_OK;
}

int zfft_history_shape(const zfft_plan *p, int64_t *capacity, int32_t *cols, int32_t *format) {
  if (!p || !capacity || !cols || !format) return fail(ZFFT_EINVAL, "null argument");
  *capacity = p->hs_cap;
  *cols = p->hs_cap ? row_length(p) : 0;
  *format = p->hs_cap ? p->hs_q.format : 0;
  return need_on(p);
}

int zfft_history_push_device(zfft_plan *p, const float *d_rows, int32_t count, void *hip_stream) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  if (!d_rows || count < 1 || count > kMaxPushRows) return fail(ZFFT_EINVAL, "bad rows / count");
  // a push longer than the ring keeps its last hs_cap rows
  const int64_t skip = std::max<int64_t>(0, (int64_t)count - p->hs_cap);
  hipStream_t st;
  rc = begin_call(p, hip_stream, &st);
  if (rc) return rc;
  hipError_t e = launch_history_pack(d_rows + skip * p->cfg.n_win, p->cfg.n_win, (int)(count - skip),
                                     (int64_t)p->hs_seen + skip, store_of(p), st);
  if (e != hipSuccess) return hip_fail(e, "history push");
  mark(p, st, "history_pack");
  p->hs_seen += (uint64_t)count;
  return done_on(p, st);
}

int zfft_history_push(zfft_plan *p, const float *rows, int32_t count) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  if (!rows || count < 1 || count > kMaxPushRows) return fail(ZFFT_EINVAL, "bad rows / count");
  const float *d_rows;
  rc = stage_rows(p, rows, count, "history row staging", &d_rows);
  if (!rc) rc = zfft_history_push_device(p, d_rows, count, p->stream);
  if (rc) return rc;
  hipError_t e = hipStreamSynchronize(p->stream);
  return e == hipSuccess ? ZFFT_OK : hip_fail(e, "sync");
}

int zfft_history_state(zfft_plan *p, uint64_t *rows_seen, uint64_t *oldest) {
  if (!p) return fail(ZFFT_EINVAL, "null plan");
  int rc = need_on(p);
  if (rc) return rc;
  if (rows_seen) *rows_seen = p->hs_seen;
  if (oldest) *oldest = oldest_of(p);
  return ZFFT_OK;
}

int zfft_history_read_device(zfft_plan *p, int64_t first, int32_t count, float *d_rows, void *hip_stream) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  if (!d_rows || count < 1 || count > kMaxPushRows) return fail(ZFFT_EINVAL, "bad rows / count");
  if (first < 0 || (uint64_t)first < oldest_of(p) || (uint64_t)first + (uint64_t)count > p->hs_seen)
    return fail(ZFFT_EINVAL, "history read: rows outside [oldest, rows_seen)");
  hipStream_t st;
  rc = begin_call(p, hip_stream, &st);
  if (rc) return rc;
  hipError_t e = launch_history_unpack(store_of(p), first, count, p->cfg.n_win, d_rows, st);
  if (e != hipSuccess) return hip_fail(e, "history read");
  mark(p, st, "history_unpack");
  return done_on(p, st);
}

int zfft_history_read(zfft_plan *p, int64_t first, int32_t count, float *rows_out) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  if (!rows_out || count < 1 || count > kMaxPushRows) return fail(ZFFT_EINVAL, "bad rows / count");
  const size_t cells = (size_t)count * p->cfg.n_win;
  rc = grow(p, p->row_stage, cells * sizeof(float), "history row staging");
  if (rc) return rc;
  rc = use_stream(p, p->stream);
  if (rc) return rc;
  if (row_length(p) < p->cfg.n_win) {  // the columns at or beyond the row length read as NaN
    hipError_t e = launch_view_fill(p->row_stage.as<float>(), (int64_t)cells, kNaN, p->stream);
    if (e != hipSuccess) return hip_fail(e, "history fill");
    rc = done_on(p, p->stream);
    if (rc) return rc;
  }
  rc = zfft_history_read_device(p, first, count, p->row_stage.as<float>(), p->stream);
  if (rc) return rc;
  hipError_t e = hipMemcpyAsync(rows_out, p->row_stage.p, cells * sizeof(float), hipMemcpyDeviceToHost, p->stream);
  return sync_read(p, e, "history read");
}

int zfft_history_view_device(zfft_plan *p, const zfft_history_window *w, float *d_img, void *hip_stream) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  rc = window_ok(p, w);
  if (rc) return rc;
  if (!d_img) return fail(ZFFT_EINVAL, "null output");
  HistGeom g{};
  g.first = w->first;
  g.oldest = (int64_t)oldest_of(p);
  g.seen = (int64_t)p->hs_seen;
  g.col0 = w->col0;
  g.span = w->col1 - w->col0;
  g.width = w->width;
  g.det = w->detector;
  g.m = w->rows_per_line;
  g.lines = w->lines;
  const HistForm f = choose_history(g.lines, g.m, g.span, g.width, p->hs_q.format);
  if (!f.ok()) return fail(ZFFT_EINTERNAL, "history: no form for this window");
  rc = grow(p, p->hs_scratch, history_scratch_bytes(f, g.width), "history scratch");
  if (rc) return rc;
  hipStream_t st;
  rc = begin_call(p, hip_stream, &st);
  if (rc) return rc;
  const HistStore s = store_of(p);
  hipError_t e = launch_history_view(s, g, f, d_img, p->hs_scratch.p, p->hs_scratch.cap, st);
  if (e != hipSuccess) return hip_fail(e, "history view");
  mark(p, st, "history_view");
  if (f.kind == kHistSliced) {
    e = launch_history_finish(s, g, f, d_img, p->hs_scratch.p, p->hs_scratch.cap, st);
    if (e != hipSuccess) return hip_fail(e, "history finish");
    mark(p, st, "history_finish");
  }
  p->hs_kind = f.kind;
  return done_on(p, st);
}

int zfft_history_view(zfft_plan *p, const zfft_history_window *w, float *img_out) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  rc = window_ok(p, w);
  if (rc) return rc;
  if (!img_out) return fail(ZFFT_EINVAL, "null output");
  const size_t bytes = (size_t)w->lines * w->width * sizeof(float);
  rc = grow(p, p->hs_img, bytes, "history image");
  if (rc) return rc;
  rc = zfft_history_view_device(p, w, p->hs_img.as<float>(), p->stream);
  if (rc) return rc;
  hipError_t e = hipMemcpyAsync(img_out, p->hs_img.p, bytes, hipMemcpyDeviceToHost, p->stream);
  return sync_read(p, e, "history view");
}

int zfft_history_render(zfft_plan *p, const zfft_history_window *w, uint8_t *rgba_out) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  rc = window_ok(p, w);
  if (rc) return rc;
  if (!rgba_out) return fail(ZFFT_EINVAL, "null output");
  const size_t px = (size_t)w->lines * w->width;
  rc = grow(p, p->hs_img, px * sizeof(float), "history image");
  if (!rc) rc = grow(p, p->hs_rgba, px * 4, "history pixel");
  if (rc) return rc;
  rc = zfft_history_view_device(p, w, p->hs_img.as<float>(), p->stream);
  if (rc) return rc;
  double lo, scale;
  rc = render_setup(p, p->stream, &lo, &scale);
  if (rc) return rc;
  // the view is in image order already: a ring of `lines` lines read from offset 0
  hipError_t e = launch_waterfall_render(p->hs_img.as<float>(), w->lines, w->width, 0, p->lut_d.p, lo, scale,
                                         p->hs_rgba.p, p->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(rgba_out, p->hs_rgba.p, px * 4, hipMemcpyDeviceToHost, p->stream);
  return sync_read(p, e, "history render");
}

int zfft_history_replay_viewport(zfft_plan *p, int64_t first) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  if (!p->vw_h) return fail(ZFFT_EINVAL, "history replay: the viewport is off (zfft_plan_viewport)");
  rc = zfft_viewport_reset(p);
  if (rc) return rc;
  int64_t at = std::max<int64_t>(first, (int64_t)oldest_of(p));
  const int64_t end = (int64_t)p->hs_seen;
  if (at < end) {
    const size_t row_bytes = (size_t)p->cfg.n_win * sizeof(float);
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>((int64_t)(kReplayChunk / row_bytes), end - at));
    rc = grow(p, p->hs_replay, (size_t)chunk * row_bytes, "history replay scratch");
    if (rc) return rc;
    if (row_length(p) < p->cfg.n_win) {  // (never read by the viewport; defined all the same)
      rc = use_stream(p, p->stream);
      if (rc) return rc;
      hipError_t e = launch_view_fill(p->hs_replay.as<float>(), chunk * p->cfg.n_win, kNaN, p->stream);
      if (e != hipSuccess) return hip_fail(e, "history replay fill");
      rc = done_on(p, p->stream);
      if (rc) return rc;
    }
    // unpack and push alternate on the plan's stream: each chunk's push has read the scratch
    // before the next chunk's unpack overwrites it
    for (; at < end; at += chunk) {
      const int32_t cnt = (int32_t)std::min<int64_t>(chunk, end - at);
      rc = zfft_history_read_device(p, at, cnt, p->hs_replay.as<float>(), p->stream);
      if (!rc) rc = zfft_viewport_push_device(p, p->hs_replay.as<float>(), cnt, p->stream);
      if (rc) return rc;
    }
  }
  hipError_t e = hipStreamSynchronize(p->stream);
  return e == hipSuccess ? ZFFT_OK : hip_fail(e, "sync");
}

int zfft_history_reset(zfft_plan *p) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  p->hs_seen = 0;  // (what the slots hold is never read before it is written again)
  return ZFFT_OK;
}

}  // extern "C"
