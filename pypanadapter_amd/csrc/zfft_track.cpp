// zfft_track.cpp -- the emission tracker of libzfft.so: the detector's runs linked across rows
// into tracks, with the state carried from push to push on the device (C-ABI and rule: zfft.h;
// kernels: track_kernels.hip; form chooser: zfft_track_plan.h).  The model is
// zfft_detect.cpp's: nothing runs inside zfft_process*.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "zfft.h"
#include "zfft_plan.h"

using namespace zfft;

namespace {

// the carried state in tk_state
constexpr size_t kOffCtr = 0, kOffFound = 64, kOffParent = 128, kOffEv = kOffParent + 4 * kTrackFrontier,
                 kOffOpen = kOffEv + 16 * kTrackFrontier, kStateBytes = kOffOpen + sizeof(TrackOpen) * kTrackFrontier;
static_assert(sizeof(TrackCounters) <= 64 && sizeof(zfft_emission) == 16 && sizeof(zfft_track) == 64, "layout");

int need_on(const zfft_plan *p) {
  return p->tk_max ? ZFFT_OK : fail(ZFFT_EINVAL, "tracking is off (zfft_plan_track)");
}

// The arguments every launch shares; the pass's part (R, chunks, found, events, scratch) is the caller's.
TrackArgs base_args(const zfft_plan *p) {
  TrackArgs a{};
  char *s = p->tk_state.as<char>();
  a.K = p->dt_k, a.G = p->tk_gap + 1, a.slack = p->tk_slack, a.min_rows = p->tk_min_rows, a.max_tracks = p->tk_max;
  a.head = p->tk_head;
  a.ctr = (TrackCounters *)(s + kOffCtr);
  a.fr_found = (int32_t *)(s + kOffFound);
  a.fr_parent = (uint32_t *)(s + kOffParent);
  a.fr_ev = (zfft_emission *)(s + kOffEv);
  a.open_tab = (TrackOpen *)(s + kOffOpen);
  a.store = p->tk_store.as<zfft_track>();
  return a;
}

// Everything back to zero on the plan's stream: the state cleared, the frontier's parents set.
int restart(zfft_plan *p) {
  int rc = use_stream(p, p->stream);
  if (rc) return rc;
  hipError_t e = hipMemsetAsync(p->tk_state.p, 0, kStateBytes, p->stream);
  if (e == hipSuccess) e = launch_track_flush(base_args(p), p->stream);  // (nothing is open: it only sets the parents)
  if (e != hipSuccess) return hip_fail(e, "track reset");
  p->tk_rows = 0;
  p->tk_head = 0;
  return done_on(p, p->stream);
}

// Waits for the plan's work and reads the counters.
int read_counters(zfft_plan *p, TrackCounters *c) {
  int rc = use_stream(p, p->stream);
  if (rc) return rc;
  hipError_t e = hipMemcpyAsync(c, p->tk_state.as<char>() + kOffCtr, sizeof(*c), hipMemcpyDeviceToHost, p->stream);
  return sync_read(p, e, "track counters read");
}

}  // namespace

namespace zfft {

void track_release(zfft_plan *p) {
  p->tk_state.release();
  p->tk_store.release();
  p->tk_scratch.release();
  p->tk_stage.release();
  p->tk_max = 0;
  p->tk_rows = 0;
  p->tk_head = 0;
}

int track_restart(zfft_plan *p) { return p->tk_max ? restart(p) : ZFFT_OK; }

}  // namespace zfft

// Test hook (not part of include/zfft.h): {chunk_rows, pass_rows, passes, chunks} of a push of
// `count` rows on this plan.
extern "C" int zfft__plan_track_form(const zfft_plan *p, int32_t count, int32_t *out4) {
  if (!p || !out4 || !p->tk_max) return ZFFT_EINVAL;
  const TrackForm f = choose_track(p->dt_k, p->tk_gap, count);
  if (!f.ok()) return ZFFT_EINVAL;
  out4[0] = f.chunk_rows, out4[1] = f.pass_rows, out4[2] = f.passes, out4[3] = f.chunks;
  return ZFFT_OK;
}

extern "C" {

int zfft_plan_track(zfft_plan *p, int32_t gap, int32_t slack, int32_t min_rows, int32_t max_tracks) {
  int rc = enter(p);
  if (rc) return rc;
  if (max_tracks == 0) {
    rc = quiesce(p);  // an enqueued push may still use all of it
    if (rc) return rc;
    track_release(p);
    return ZFFT_OK;
  }
  if (!p->dt_k) return fail(ZFFT_EINVAL, "track: detection is off (zfft_plan_detect)");
  if (gap < 0 || gap > kTrackMaxGap || slack < 0 || slack > kTrackMaxSlack || min_rows < 1 || max_tracks < 1 ||
      max_tracks > kTrackMaxTracks)
    return fail(ZFFT_EINVAL, "track: gap in [0, 7], slack in [0, 64], min_rows >= 1, max_tracks 0 (off) or in [1, 2^22]");
  rc = quiesce(p);  // the store may be replaced under an enqueued push
  if (rc) return rc;
  if (p->tk_state.ensure(kStateBytes) != hipSuccess ||
      p->tk_store.ensure((size_t)max_tracks * sizeof(zfft_track)) != hipSuccess) {
    track_release(p);
    return fail(ZFFT_ENOMEM, "track allocation failed");
  }
  p->tk_gap = gap, p->tk_slack = slack, p->tk_min_rows = min_rows, p->tk_max = max_tracks;
  return restart(p);
}

int zfft_track_shape(const zfft_plan *p, int32_t *gap, int32_t *slack, int32_t *min_rows, int32_t *max_tracks) {
  if (!p || !gap || !slack || !min_rows || !max_tracks) return fail(ZFFT_EINVAL, "null argument");
  *gap = p->tk_gap, *slack = p->tk_slack, *min_rows = p->tk_min_rows, *max_tracks = p->tk_max;
  return need_on(p);
}

int zfft_track_push_device(zfft_plan *p, const int32_t *d_found, const zfft_emission *d_events, int32_t count,
                           void *hip_stream) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  if (!d_found || !d_events || count < 1 || count > kMaxDetectRows) return fail(ZFFT_EINVAL, "bad found / records / count");
  const int K = p->dt_k, gap = p->tk_gap;
  const TrackForm f = choose_track(K, gap, count);
  if (!f.ok()) return fail(ZFFT_EINVAL, "track: no form for this call");
  const int rows0 = std::min(count, f.pass_rows);
  rc = grow(p, p->tk_scratch, track_scratch_bytes(K, gap, rows0), "track scratch");
  if (rc) return rc;
  hipStream_t st;
  rc = begin_call(p, hip_stream, &st);
  if (rc) return rc;
  TrackArgs a = base_args(p);
  for (int off = 0; off < count; off += f.pass_rows) {  // (one stream: a pass reuses the scratch after the last)
    a.R = std::min(f.pass_rows, count - off);
    a.chunk_rows = f.chunk_rows;
    a.chunks = f.chunks_of(a.R);
    a.t0 = (int64_t)p->tk_rows;
    a.found = d_found + off;
    a.events = d_events + (int64_t)off * K;
    // the scratch: the aggregates first (zeroed as one block), then the parents and the rows' counts
    const size_t nodes = (size_t)(a.R + a.G) * K, lrows = (size_t)a.R + a.G;
    char *s = p->tk_scratch.as<char>();
    a.a_name = (uint64_t *)s, a.a_last = a.a_name + nodes, a.a_cells = a.a_last + nodes, a.a_runs = a.a_cells + nodes;
    a.a_prow = a.a_runs + nodes;
    a.a_colf = (uint32_t *)(a.a_prow + nodes), a.a_coll = a.a_colf + nodes, a.a_pkey = a.a_coll + nodes;
    a.a_pcol = a.a_pkey + nodes;
    a.c_prow = (uint64_t *)(a.a_pcol + nodes);
    a.c_pkey = (uint32_t *)(a.c_prow + nodes), a.c_pcol = a.c_pkey + nodes;
    a.parent = a.c_pcol + nodes;
    a.rowcnt = (int32_t *)(a.parent + nodes), a.rowoff = a.rowcnt + lrows;
    hipError_t e = hipMemsetAsync(s, 0, nodes * 56, st);
    if (e != hipSuccess) return hip_fail(e, "track scratch clear");
    for (int step = 0; step < kTrackSteps; ++step) {
      e = launch_track_step(step, a, st);
      if (e != hipSuccess) return hip_fail(e, kTrackStepNames[step]);
      mark(p, st, kTrackStepNames[step]);
    }
    p->tk_rows += (uint64_t)a.R;
  }
  return done_on(p, st);
}

int zfft_track_push(zfft_plan *p, const int32_t *found, const zfft_emission *events, int32_t count) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  if (!found || !events || count < 1 || count > kMaxDetectRows) return fail(ZFFT_EINVAL, "bad found / records / count");
  const int K = p->dt_k;
  for (int64_t r = 0; r < count; ++r) {  // rule 9 on the slots the tracker will use
    const int used = std::min(std::max(found[r], 0), K);
    int64_t prev = -1;
    for (int s = 0; s < used; ++s) {
      const zfft_emission &e = events[r * K + s];
      if (!((int64_t)e.first > prev && e.first <= e.peak && e.peak <= e.last) || std::isnan(e.peak_db))
        return fail(ZFFT_EINVAL, "track: records must be ascending, disjoint, 0 <= first <= peak <= last, peak_db not NaN");
      prev = e.last;
    }
  }
  const size_t ev_bytes = (size_t)count * K * sizeof(zfft_emission), n4 = (size_t)count * 4;
  rc = grow(p, p->tk_stage, ev_bytes + n4, "track staging");
  if (!rc) rc = use_stream(p, p->stream);  // the staging may still be read by the previous call
  if (rc) return rc;
  char *d = p->tk_stage.as<char>();
  hipError_t e = hipMemcpyAsync(d, events, ev_bytes, hipMemcpyHostToDevice, p->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d + ev_bytes, found, n4, hipMemcpyHostToDevice, p->stream);
  if (e != hipSuccess) return hip_fail(e, "H2D records");
  rc = zfft_track_push_device(p, (const int32_t *)(d + ev_bytes), (const zfft_emission *)d, count, p->stream);
  if (rc) return rc;
  e = hipStreamSynchronize(p->stream);
  return e == hipSuccess ? ZFFT_OK : hip_fail(e, "track push");
}

int zfft_track_read(zfft_plan *p, zfft_track *out, int32_t max, int32_t *n) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  if (!n || max < 0 || (max > 0 && !out)) return fail(ZFFT_EINVAL, "bad output / max");
  TrackCounters c;
  rc = read_counters(p, &c);
  if (rc) return rc;
  const uint32_t cap = (uint32_t)p->tk_max, take = (uint32_t)std::min<uint64_t>(c.unread, (uint64_t)max);
  *n = (int32_t)take;
  if (!take) return ZFFT_OK;
  const uint32_t n1 = std::min(take, cap - p->tk_head);  // up to the ring's end, then from its start
  const zfft_track *store = p->tk_store.as<zfft_track>();
  hipError_t e = hipMemcpy(out, store + p->tk_head, (size_t)n1 * sizeof(zfft_track), hipMemcpyDeviceToHost);
  if (e == hipSuccess && take > n1)
    e = hipMemcpy(out + n1, store, (size_t)(take - n1) * sizeof(zfft_track), hipMemcpyDeviceToHost);
  const uint64_t left = c.unread - take;
  if (e == hipSuccess)
    e = hipMemcpy(p->tk_state.as<char>() + kOffCtr + offsetof(TrackCounters, unread), &left, sizeof(left),
                  hipMemcpyHostToDevice);
  if (e != hipSuccess) return hip_fail(e, "track read");
  p->tk_head = (p->tk_head + take) % cap;
  return ZFFT_OK;
}

int zfft_track_open(zfft_plan *p, zfft_track *out, int32_t max, int32_t *n) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  if (!n || max < 0 || (max > 0 && !out)) return fail(ZFFT_EINVAL, "bad output / max");
  rc = quiesce(p);
  if (rc) return rc;
  std::vector<char> h(kStateBytes);
  hipError_t e = hipMemcpy(h.data(), p->tk_state.p, kStateBytes, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return hip_fail(e, "track open read");
  *n = track_open_records((const int32_t *)(h.data() + kOffFound), (const uint32_t *)(h.data() + kOffParent),
                          (const TrackOpen *)(h.data() + kOffOpen), p->dt_k, p->tk_gap + 1, out, max);
  return ZFFT_OK;
}

int zfft_track_flush(zfft_plan *p) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  rc = use_stream(p, p->stream);
  if (rc) return rc;
  hipError_t e = launch_track_flush(base_args(p), p->stream);
  if (e != hipSuccess) return hip_fail(e, "track flush");
  rc = done_on(p, p->stream);
  if (rc) return rc;
  e = hipStreamSynchronize(p->stream);
  return e == hipSuccess ? ZFFT_OK : hip_fail(e, "track flush");
}

int zfft_track_state(zfft_plan *p, zfft_track_stats *out) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  if (!out) return fail(ZFFT_EINVAL, "null output");
  TrackCounters c;
  rc = read_counters(p, &c);
  if (rc) return rc;
  out->rows_seen = p->tk_rows, out->open = c.open, out->unread = c.unread, out->dropped = c.dropped;
  out->short_tracks = c.short_tracks, out->truncated_rows = c.truncated_rows;
  return ZFFT_OK;
}

int zfft_track_reset(zfft_plan *p) {
  int rc = enter(p);
  if (rc) return rc;
  rc = need_on(p);
  if (rc) return rc;
  return restart(p);
}

}  // extern "C"
