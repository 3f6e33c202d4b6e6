// zfft_detect.cpp -- the row detector of libzfft.so: per row a noise floor, the emissions above
// floor + threshold and a per-column occupancy count, from rows the caller holds on the device
// (C-ABI and rule: zfft.h; kernel: detect_kernels.hip; form chooser: zfft_detect_plan.h;
// DESIGN §3.3.4).  The model is zfft_persist.cpp's: nothing runs inside zfft_process*.
// zfft_plan_detect_local switches the on-flags to a floor per column (detect_local_kernels.hip;
// DESIGN §3.3.7): the floors of a pass go through the plan's scratch dt_floors, then the same
// detect_rows kernel reads them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>

#include "zfft.h"
#include "zfft_plan.h"

using namespace zfft;

namespace {

// The detector's rows are the plan's (zfft_plan_row_length) unless the test hook gave a length.
int det_length(const zfft_plan *p) { return p->dt_row_len ? p->dt_row_len : row_length(p); }

int need_on(const zfft_plan *p) {
  return p->dt_k ? ZFFT_OK : fail(ZFFT_EINVAL, "detection is off (zfft_plan_detect)");
}

int zero_occupancy(zfft_plan *p) {
  int rc = use_stream(p, p->stream);
  if (rc) return rc;
  hipError_t e = hipMemsetAsync(p->dt_occ.p, 0, (size_t)p->cfg.n_win * sizeof(unsigned), p->stream);
  if (e != hipSuccess) return hip_fail(e, "detect reset");
  p->dt_rows = 0;
  return done_on(p, p->stream);
}

int need_local(const zfft_plan *p) {
  return p->dt_h ? ZFFT_OK : fail(ZFFT_EINVAL, "the floor is row-global (zfft_plan_detect_local)");
}

// The local floors of `count` device rows into dst (rows of dst_stride floats), in passes of
// the form's chunk_rows; one launch per pass on st.
int run_floors(zfft_plan *p, const float *d_rows, int count, float *dst, int64_t dst_stride, size_t cap,
               hipStream_t st) {
  const int n_win = p->cfg.n_win, n = det_length(p);
  for (int off = 0; off < count;) {
    const DetectLocalForm f = choose_detect_local(n, n_win, count - off, p->dt_h, p->dt_guard, cap);
    if (!f.ok()) return fail(ZFFT_EINVAL, "detect: no local form for this plan");
    hipError_t e = launch_detect_floors(d_rows + (int64_t)off * n_win, n_win, f.chunk_rows, n, p->dt_h, p->dt_guard,
                                        p->dt_q, f, dst + (int64_t)off * dst_stride, dst_stride, st);
    if (e != hipSuccess) return hip_fail(e, "detect floors");
    off += f.chunk_rows;
  }
  return ZFFT_OK;
}

}  // namespace

// Test hooks (not part of include/zfft.h): the local floor's form for a call on `count` rows of
// this plan, as zfft__detect_local_form gives it; and the cap of the floors scratch in bytes
// (0 = the default), so that a small call runs in several passes.
extern "C" int zfft__plan_detect_local_form(const zfft_plan *p, int32_t count, int32_t *out7) {
  if (!p || !out7 || !p->dt_h) return ZFFT_EINVAL;
  const DetectLocalForm f = choose_detect_local(det_length(p), p->cfg.n_win, count, p->dt_h, p->dt_guard, p->dt_local_cap);
  if (!f.ok()) return ZFFT_EINVAL;
  out7[0] = f.tile, out7[1] = f.tiles, out7[2] = f.halo, out7[3] = f.grid, out7[4] = f.chunk_rows;
  out7[5] = f.lds_keys(), out7[6] = f.words;
  return ZFFT_OK;
}
// Test hook: the row length the detector takes its rows to have, 1 <= n <= n_win (0 = the plan's
// own): a plan's rows are at least two columns and of few shapes, the kernels' edge cases are not.
extern "C" int zfft__plan_detect_row_length(zfft_plan *p, int32_t n) {
  if (!p || n < 0 || n > p->cfg.n_win) return ZFFT_EINVAL;
  p->dt_row_len = n;
  return ZFFT_OK;
}
extern "C" int zfft__plan_detect_local_cap(zfft_plan *p, int64_t bytes) {
  if (!p || bytes < 0) return ZFFT_EINVAL;
  p->dt_local_cap = (size_t)bytes;
  return ZFFT_OK;
}

// Test hook (not part of include/zfft.h): the form a call on `count` rows of this plan takes.
extern "C" int zfft__plan_detect_form(const zfft_plan *p, int32_t count, int32_t *waves, int32_t *per,
                                      int32_t *grid) {
  if (!p || !waves || !per || !grid) return ZFFT_EINVAL;
  const DetectForm f = choose_detect(det_length(p), count);
  if (!f.ok()) return ZFFT_EINVAL;
  *waves = f.waves;
  *per = f.per;
  *grid = f.grid;
  return ZFFT_OK;
}

extern "C" {

int zfft_plan_detect(zfft_plan *p, double quantile, double threshold_db, int32_t min_width,
                     int32_t max_per_row) {
  int rc = enter(p);
  if (rc) return rc;
  if (max_per_row == 0) {
    rc = quiesce(p);  // an enqueued call may still add to the table and read the staging
    if (rc) return rc;
    p->dt_occ.release();
    p->row_stage.release();
    p->dt_out.release();
    p->dt_floors.release();
    track_release(p);  // tracking belongs to the detector
    p->dt_k = 0;
    p->dt_rows = 0;
    p->dt_h = p->dt_guard = 0;  // the next zfft_plan_detect starts row-global
    return ZFFT_OK;
  }
  if (max_per_row < 1 || max_per_row > kDetectMaxPerRow || !(quantile >= 0.0 && quantile <= 1.0) ||
      !std::isfinite(threshold_db) || min_width < 1 || min_width > p->cfg.n_win)
    return fail(ZFFT_EINVAL, "detect: max_per_row 0 (off) or in [1, 32], quantile in [0, 1], threshold_db "
                             "finite, min_width in [1, n_win]");
  if (p->dt_occ.ensure((size_t)p->cfg.n_win * sizeof(unsigned)) != hipSuccess) {  // (n_win is the plan's: never grows)
    p->dt_k = 0;
    return fail(ZFFT_ENOMEM, "detect occupancy allocation failed");
  }
  const bool new_k = p->dt_k != max_per_row;
  p->dt_k = max_per_row;
  p->dt_q = quantile;
  p->dt_thr = (float)threshold_db;
  p->dt_min_width = min_width;
  rc = zero_occupancy(p);
  if (rc || !new_k) return rc;
  return track_restart(p);  // the tracker's rows had another K (nothing to do while it is off)
}

int zfft_plan_detect_local(zfft_plan *p, int32_t half_window, int32_t guard) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  if (half_window == 0 ? guard != 0
                       : (half_window < 1 || half_window > kDetectLocalMaxHalf || guard < 0 ||
                          guard > kDetectLocalMaxGuard))
    return fail(ZFFT_EINVAL, "detect local: half_window 0 (row-global; guard 0) or in [1, 128], guard in [0, 128]");
  if (half_window == 0 && p->dt_floors.p) {
    rc = quiesce(p);  // an enqueued call may still read the floors
    if (rc) return rc;
    p->dt_floors.release();
  }
  p->dt_h = half_window;
  p->dt_guard = guard;
  return zero_occupancy(p);  // counts made under two rules do not add
}

int zfft_detect_local_shape(const zfft_plan *p, int32_t *half_window, int32_t *guard) {
  if (!p || !half_window || !guard) return fail(ZFFT_EINVAL, "null argument");
  *half_window = p->dt_h;
  *guard = p->dt_guard;
  return need_on(p);
}

int zfft_detect_shape(const zfft_plan *p, int32_t *max_per_row, int32_t *cols) {
  if (!p || !max_per_row || !cols) return fail(ZFFT_EINVAL, "null argument");
  *max_per_row = p->dt_k;
  *cols = p->cfg.n_win;
  return need_on(p);
}

int zfft_detect_device(zfft_plan *p, const float *d_rows, int32_t count, float *d_floor, int32_t *d_found,
                       zfft_emission *d_events, void *hip_stream) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  if (!d_rows || !d_floor || !d_found || !d_events || count < 1 || count > kMaxDetectRows)
    return fail(ZFFT_EINVAL, "bad rows / outputs / count");
  if ((uintptr_t)d_events & 15) return fail(ZFFT_EINVAL, "detect: the records must be 16-byte aligned");
  const DetectGeom g{p->cfg.n_win, det_length(p), p->dt_q, p->dt_thr, p->dt_min_width, p->dt_k};
  const DetectForm f = choose_detect(g.row_len, count);
  if (!f.ok()) return fail(ZFFT_EINVAL, "detect: the plan's rows are empty");
  hipStream_t st = pick_stream(p, hip_stream);
  if (p->dt_h) {  // a floor per column: floors into the scratch, then the rows against them, pass by pass
    const int n_win = p->cfg.n_win;
    const DetectLocalForm lf = choose_detect_local(g.row_len, n_win, count, p->dt_h, p->dt_guard, p->dt_local_cap);
    if (!lf.ok()) return fail(ZFFT_EINVAL, "detect: no local form for this plan");
    const size_t need = (size_t)lf.chunk_rows * n_win * sizeof(float);
    rc = grow(p, p->dt_floors, need, "detect floors");
    if (!rc) rc = use_stream(p, st);
    if (rc) return rc;
    p->dt_rows += (uint64_t)count;
    p->n_marks = 0;
    mark(p, st, "start");
    for (int off = 0; off < count; off += lf.chunk_rows) {  // (one stream: a pass reuses the scratch after the last)
      const int cnt = std::min(lf.chunk_rows, count - off);
      const float *r = d_rows + (int64_t)off * n_win;
      rc = run_floors(p, r, cnt, p->dt_floors.as<float>(), n_win, need, st);
      if (rc) return rc;
      mark(p, st, "detect_floor");
      hipError_t e = launch_detect_rows(r, n_win, cnt, g, choose_detect(g.row_len, cnt), d_floor + off, d_found + off,
                                        d_events + (int64_t)off * p->dt_k, p->dt_occ.as<unsigned>(), st,
                                        p->dt_floors.as<float>());
      if (e != hipSuccess) return hip_fail(e, "detect");
      mark(p, st, "detect_rows");
    }
    return done_on(p, st);
  }
  rc = use_stream(p, st);  // after the table's zeroing and earlier calls, on any stream
  if (rc) return rc;
  p->dt_rows += (uint64_t)count;
  p->n_marks = 0;
  mark(p, st, "start");
  hipError_t e = launch_detect_rows(d_rows, p->cfg.n_win, count, g, f, d_floor, d_found, d_events,
                                    p->dt_occ.as<unsigned>(), st);
  if (e != hipSuccess) return hip_fail(e, "detect");
  mark(p, st, "detect_rows");
  return done_on(p, st);
}

int zfft_detect(zfft_plan *p, const float *rows, int32_t count, float *floor_out, int32_t *found_out,
                zfft_emission *events_out) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  if (!rows || !floor_out || !found_out || !events_out || count < 1 || count > kMaxDetectRows)
    return fail(ZFFT_EINVAL, "bad rows / outputs / count");
  // the records first (16-byte aligned), then the floors, then the counts
  const size_t ev_bytes = (size_t)count * p->dt_k * sizeof(zfft_emission), n4 = (size_t)count * 4;
  const float *d_rows;
  rc = grow(p, p->dt_out, ev_bytes + 2 * n4, "detect staging");
  if (!rc) rc = stage_rows(p, rows, count, "detect staging", &d_rows);
  if (rc) return rc;
  char *out = p->dt_out.as<char>();
  rc = zfft_detect_device(p, d_rows, count, (float *)(out + ev_bytes), (int32_t *)(out + ev_bytes + n4),
                          (zfft_emission *)out, p->stream);
  if (rc) return rc;
  hipError_t e = hipMemcpyAsync(events_out, out, ev_bytes, hipMemcpyDeviceToHost, p->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(floor_out, out + ev_bytes, n4, hipMemcpyDeviceToHost, p->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(found_out, out + ev_bytes + n4, n4, hipMemcpyDeviceToHost, p->stream);
  return sync_read(p, e, "detect D2H");
}

int zfft_detect_floors_device(zfft_plan *p, const float *d_rows, int32_t count, float *d_floors, void *hip_stream) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  rc = need_local(p);
  if (rc) return rc;
  if (!d_rows || !d_floors || count < 1 || count > kMaxDetectRows) return fail(ZFFT_EINVAL, "bad rows / output / count");
  hipStream_t st;
  rc = begin_call(p, hip_stream, &st);
  if (rc) return rc;
  // straight into the caller's rows: no scratch; the cap only sets the rows of a launch
  rc = run_floors(p, d_rows, count, d_floors, p->cfg.n_win, p->dt_local_cap, st);
  if (rc) return rc;
  mark(p, st, "detect_floor");
  return done_on(p, st);
}

int zfft_detect_floors(zfft_plan *p, const float *rows, int32_t count, float *floors_out) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  rc = need_local(p);
  if (rc) return rc;
  if (!rows || !floors_out || count < 1 || count > kMaxDetectRows) return fail(ZFFT_EINVAL, "bad rows / output / count");
  const int n_win = p->cfg.n_win, n = det_length(p);
  const size_t bytes = (size_t)count * n_win * sizeof(float);
  const float *d_rows;
  rc = grow(p, p->dt_out, bytes, "detect staging");
  if (!rc) rc = stage_rows(p, rows, count, "detect staging", &d_rows);
  if (!rc) rc = zfft_detect_floors_device(p, d_rows, count, p->dt_out.as<float>(), p->stream);
  if (rc) return rc;
  rc = sync_read(p, hipMemcpyAsync(floors_out, p->dt_out.p, bytes, hipMemcpyDeviceToHost, p->stream),
                 "detect floors D2H");
  if (rc) return rc;
  for (int64_t r = 0; r < count; ++r)  // the device leaves the columns beyond the row untouched
    std::fill(floors_out + r * n_win + n, floors_out + (r + 1) * n_win, std::numeric_limits<float>::quiet_NaN());
  return ZFFT_OK;
}

int zfft_detect_occupancy(zfft_plan *p, uint32_t *occ_out, uint64_t *rows_seen) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  if (!occ_out) return fail(ZFFT_EINVAL, "null output");
  rc = use_stream(p, p->stream);
  if (rc) return rc;
  hipError_t e = hipMemcpyAsync(occ_out, p->dt_occ.p, (size_t)p->cfg.n_win * sizeof(unsigned),
                                hipMemcpyDeviceToHost, p->stream);
  rc = sync_read(p, e, "detect occupancy read");
  if (rc) return rc;
  if (rows_seen) *rows_seen = p->dt_rows;
  return ZFFT_OK;
}

int zfft_detect_reset(zfft_plan *p) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  return zero_occupancy(p);
}

}  // extern "C"
