// zfft_persist.cpp -- the persistence spectrum of libzfft.so: a per-column histogram of the levels
// of the rows the caller pushes, kept on the device (C-ABI and binning rule: zfft.h; kernel:
// zfft_kernels.hip persist_hist_kernel).
#include <hip/hip_runtime.h>

#include <cmath>

#include "zfft.h"
#include "zfft_plan.h"

using namespace zfft;

namespace {

constexpr int kMaxLevels = 256;         // 64 KB of LDS counters per workgroup

int need_on(const zfft_plan *p) {
  return p->ps_levels ? ZFFT_OK : fail(ZFFT_EINVAL, "persistence is off (zfft_plan_persistence)");
}

size_t table_cells(const zfft_plan *p) { return (size_t)p->ps_levels * p->cfg.n_win; }

int zero_table(zfft_plan *p) {
  int rc = use_stream(p, p->stream);
  if (rc) return rc;
  hipError_t e = hipMemsetAsync(p->ps_hist.p, 0, table_cells(p) * sizeof(unsigned), p->stream);
  if (e != hipSuccess) return hip_fail(e, "persistence reset");
  p->ps_rows = 0;
  return done_on(p, p->stream);
}

}  // namespace

// Test hook (not part of include/zfft.h): the row slices of the plan's last persistence push.
extern "C" int zfft__plan_persist_slices(const zfft_plan *p) { return p ? p->ps_slices : -1; }

extern "C" {

int zfft_plan_persistence(zfft_plan *p, int32_t levels, double db_min, double db_max) {
  int rc = enter(p);
  if (rc) return rc;
  if (levels == 0) {
    rc = quiesce(p);  // an enqueued push may still add to the table
    if (rc) return rc;
    p->ps_hist.release();
    p->row_stage.release();
    p->ps_levels = 0;
    p->ps_rows = 0;
    return ZFFT_OK;
  }
  if (levels < 2 || levels > kMaxLevels || !std::isfinite(db_min) || !std::isfinite(db_max) ||
      !(db_min < db_max))
    return fail(ZFFT_EINVAL, "persistence: levels 0 (off) or in [2, 256], db_min < db_max finite");
  const float inv = (float)((double)levels / (db_max - db_min));
  if (!std::isfinite(inv) || !std::isfinite((float)db_min))
    return fail(ZFFT_EINVAL, "persistence: the level width does not fit float32");
  rc = grow(p, p->ps_hist, (size_t)levels * p->cfg.n_win * sizeof(unsigned), "persistence table");
  if (rc == ZFFT_ENOMEM) p->ps_levels = 0;
  if (rc) return rc;
  p->ps_levels = levels;
  p->ps_lo = (float)db_min;
  p->ps_inv = inv;
  return zero_table(p);
}

int zfft_persistence_shape(const zfft_plan *p, int32_t *levels, int32_t *cols) {
  if (!p || !levels || !cols) return fail(ZFFT_EINVAL, "null argument");
  *levels = p->ps_levels;
  *cols = p->cfg.n_win;
  return need_on(p);
}

int zfft_persistence_push_device(zfft_plan *p, const float *d_rows, int32_t count, void *hip_stream) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  if (!d_rows || count < 1 || count > kMaxPushRows) return fail(ZFFT_EINVAL, "bad rows / count");
  hipStream_t st = pick_stream(p, hip_stream);
  rc = use_stream(p, st);  // after the table's zeroing and earlier pushes, on any stream
  if (rc) return rc;
  PersistGeom g{p->cfg.n_win, row_length(p), p->ps_levels, p->ps_lo, p->ps_inv};
  p->ps_rows += (uint64_t)count;
  p->ps_slices = persist_slices(count, g.row_len);
  if (g.row_len > 0) {
    p->n_marks = 0;
    mark(p, st, "start");
    hipError_t e = launch_persist_hist(d_rows, p->cfg.n_win, count, g, p->ps_hist.as<unsigned>(), st);
    if (e != hipSuccess) return hip_fail(e, "persistence push");
    mark(p, st, "persist_hist");
  }
  return done_on(p, st);
}

int zfft_persistence_push(zfft_plan *p, const float *rows, int32_t count) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  if (!rows || count < 1 || count > kMaxPushRows) return fail(ZFFT_EINVAL, "bad rows / count");
  const float *d_rows;
  rc = stage_rows(p, rows, count, "persistence row staging", &d_rows);
  if (!rc) rc = zfft_persistence_push_device(p, d_rows, count, p->stream);
  if (rc) return rc;
  hipError_t e = hipStreamSynchronize(p->stream);
  return e == hipSuccess ? ZFFT_OK : hip_fail(e, "sync");
}

int zfft_persistence_decay(zfft_plan *p, double keep) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  if (!(keep >= 0.0 && keep <= 1.0)) return fail(ZFFT_EINVAL, "persistence decay: 0 <= keep <= 1");
  rc = use_stream(p, p->stream);
  if (rc) return rc;
  hipError_t e = launch_persist_decay(p->ps_hist.as<unsigned>(), (int64_t)table_cells(p), keep, p->stream);
  if (e != hipSuccess) return hip_fail(e, "persistence decay");
  p->ps_rows = (uint64_t)std::floor((double)p->ps_rows * keep);
  return done_on(p, p->stream);
}

int zfft_persistence_reset(zfft_plan *p) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  return zero_table(p);
}

int zfft_persistence_read(zfft_plan *p, uint32_t *hist_out, uint64_t *rows_seen) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  if (!hist_out) return fail(ZFFT_EINVAL, "null output");
  rc = use_stream(p, p->stream);
  if (rc) return rc;
  hipError_t e = hipMemcpyAsync(hist_out, p->ps_hist.p, table_cells(p) * sizeof(unsigned),
                                hipMemcpyDeviceToHost, p->stream);
  rc = sync_read(p, e, "persistence read");
  if (rc) return rc;
  if (rows_seen) *rows_seen = p->ps_rows;
  return ZFFT_OK;
}

}  // extern "C"
