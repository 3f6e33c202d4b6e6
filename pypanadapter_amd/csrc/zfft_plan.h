// zfft_plan.h -- the plan object and the helpers every host file of libzfft.so shares
// (zfft_plan.cpp, zfft_decim.cpp, zfft_welch.cpp, zfft_waterfall.cpp, zfft_persist.cpp,
// zfft_detect.cpp, zfft_track.cpp, zfft_viewport.cpp, zfft_history.cpp, zfft_stream.cpp,
// zfft_tap.cpp, zfft_chan.cpp, zfft_demod.cpp, zfft_resamp.cpp, zfft_level.cpp).  Not part of the C-ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "zfft.h"
#include "zfft_internal.h"

namespace zfft {

struct TapState;   // zfft_tap.cpp
struct ChanState;  // zfft_chan.cpp
struct DemodState;  // zfft_demod.cpp
struct ResampState;  // zfft_resamp.cpp
struct LevelState;  // zfft_level.cpp

// A grow-only device buffer, freed with its owner.
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { release(); }
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    release();
    hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
    if (e == hipSuccess) cap = bytes;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T *as() const { return static_cast<T *>(p); }
};

}  // namespace zfft

// One plan = one (N, zoom, W, window, fs, f_lo, scroll) configuration on one device, the
// analogue of the AppState fields the reference re-reads every frame
// (pypanadapter_spectrum.py:1492-1497, 2102-2119).  It owns the HIP streams, the LO /
// window / twiddle tables, a grow-only workspace and the waterfall ring; its buffers are
// freed by its destructor (zfft_plan_destroy waits for the streams first).
struct zfft_plan {
  using DevBuf = zfft::DevBuf;
  zfft_config cfg{};
  int K = 0;  // log2(zoom) decimation stages
  hipStream_t stream = nullptr;
  std::vector<float> user_window;
  DevBuf lo, win, tw, in, in2, yf, ping, pong, rows, ring, img, one_row, dec;
  hipStream_t copy_st = nullptr;            // H2D of the next batch in zfft_process
  hipEvent_t h2d_ev[2] = {}, comp_ev[2] = {};
  int64_t lo_len = 0;                       // entries per LO row (0: not built)
  std::vector<double> lo_freqs;             // set_lo_frames: one LO row per entry (config 4)
  int lo_per = 1;                           // frames per LO row
  int lo_first = 0;                         // first frame of the current batch (zfft_process)
  int win_len = -1;
  double win_ss = 0.0;
  int block_override = 0, warm_override = 0;
  int H = 0, W = 0;
  int64_t off = 0;
  bool wf_ready = false;
  const float *last_row = nullptr;  // device row of the last processed frame
  bool timing = false;
  std::vector<hipEvent_t> events;    // one per mark when timing is on
  std::vector<std::string> mark_names;
  std::string names_buf;
  int n_marks = 0;
  int path = 0;  // 0 auto, 1 exact blocked pipeline, 2 fused interior + edge windows,
                // 3 XA tiles (all-pole + FIR + half-rate all-pole), 4 PC tiles (polyphase
                // cascade; zoom 2, 4, 8 and the head of zoom >= 16), 5 PC walk (one workgroup
                // per frame; zoom 2: the tiles), 6 FC (fast convolution at zoom 4, 8 and the
                // head; where FC does not fit, as 5), 7 FC at zoom 2 and for the tails of
                // zoom >= 16 too (else as 6) -- zfft_schedule.h choose_schedule
  int welch = 0;  // 0 auto, 1 one workgroup per frame, 2 four-step -- zfft_welch_plan.h choose_welch
  DevBuf edge, xk, xa_tab, tws, means, z4, winf;
  DevBuf pc_tab, pc_edge;  // PC decimator: PcTab; all nine frame-end maps of pc_edge_maps.h
                           // (floats), uploaded once
  DevBuf pc_tab4;  // PC zoom 4: PcTab4
  DevBuf pc_tab2;  // PC zoom 2: PcTab2
  DevBuf wparts;   // split DIF Welch: partial PSDs (frames x split x n_win floats)
  // Welch detector (zfft_plan_average): ZFFT_AVG_MEAN sums the segments in the Welch kernels;
  // median / max leave every segment's bins in wsegs (frames x nseg x n_win floats, the frames
  // of a call in chunks of at most avg_cap bytes; 0 = the default cap) for welch_select
  int average = 0;
  size_t avg_cap = 0;   // test hook zfft__plan_average_cap
  DevBuf wsegs;
  // zfft_plan_segments_per_line: 0 = one row per frame; g >= 1: ceil(nseg / g) rows per frame,
  // each the detector over g consecutive segments (fused mean kernels, or reduced from wsegs)
  int seg_per_line = 0;
  int lines_route = 0;  // hook zfft__plan_lines_route: 1 = mean lines through the scratch too
  int last_split = 1;   // WelchGeom::split of the last Welch launch (test hook zfft__plan_welch_split)
  DevBuf lo1;      // unit LO table (the blocked passes after the PC head mix with it)
  int64_t lo1_n = 0;  // entries of lo1 filled (a failed fill leaves it short: refilled next call)
  int64_t n_quiesce = 0;   // host waits on enqueued work (test hook zfft__plan_quiesce_count)
  // waterfall rendering: colormap LUT (host copy + device), levels
  uint8_t lut[256 * 4] = {};
  bool lut_ready = false;         // lut holds the chosen map (built on first use)
  bool lut_uploaded = false;      // lut_d holds lut
  std::string cmap = "Default";
  double lev_lo = -220.0, lev_hi = -120.0;  // Waterfall.__init__ (S:1593-1598)
  DevBuf lut_d, rgba, al_hist, al_bins;
  DevBuf img64;                    // float64 image of the display entries
  float *row_pin = nullptr;        // page-locked staging of host rows the display kernels read
  size_t row_pin_cap = 0;          //   in place (no H2D copy command); bytes (pin_rows)
  DevBuf row_stage;                // device staging of host rows, shared by the row consumers (stage_rows)
  // persistence spectrum (zfft_plan_persistence; zfft_persist.cpp): ps_levels x n_win uint32
  // counts, level-major; 0 levels = off (no buffer).  ps_lo / ps_inv are the binning rule's
  // float32 constants; ps_rows the rows pushed (host side: pushes and decays are in call order)
  int ps_levels = 0;
  float ps_lo = 0.f, ps_inv = 0.f;
  uint64_t ps_rows = 0;
  int ps_slices = 0;               // row slices of the last push (test hook zfft__plan_persist_slices)
  DevBuf ps_hist;                  // the table
  // row detector (zfft_plan_detect; zfft_detect.cpp): dt_k = max_per_row, 0 = off (no buffer).
  // dt_occ holds n_win uint32 counts, dt_rows the rows seen (host side, in call order); dt_out
  // is the device staging of zfft_detect's outputs
  int dt_k = 0, dt_min_width = 1;
  double dt_q = 0.5;
  float dt_thr = 0.f;
  uint64_t dt_rows = 0;
  DevBuf dt_occ, dt_out;
  // the local floor (zfft_plan_detect_local): dt_h = half_window, 0 = the row-global floor (no
  // buffer).  dt_floors holds the floors of a pass, at most dt_local_cap bytes (0 = the default,
  // kDetectLocalScratch; test hook zfft__plan_detect_local_cap)
  int dt_h = 0, dt_guard = 0;
  size_t dt_local_cap = 0;
  int dt_row_len = 0;  // test hook zfft__plan_detect_row_length: the detector's row length (0 = the plan's)
  DevBuf dt_floors;
  // emission tracker (zfft_plan_track; zfft_track.cpp): tk_max = max_tracks, 0 = off (no buffer).
  // tk_state holds the carried state (frontier, open table, counters), tk_store the ring of
  // tk_max records read from tk_head, tk_scratch a pass's union-find and aggregates, tk_stage the
  // device staging of zfft_track_push's host records.  tk_rows counts the rows given (host side:
  // pushes are in call order)
  int tk_max = 0, tk_gap = 0, tk_slack = 0, tk_min_rows = 1;
  uint64_t tk_rows = 0;
  uint32_t tk_head = 0;
  DevBuf tk_state, tk_store, tk_scratch, tk_stage;
  // display viewport (zfft_plan_viewport; zfft_viewport.cpp): vw_h = 0 is off (no buffer).  A
  // ring of vw_h lines of vw_w pixels in the waterfall ring's convention (vw_off, vw_scroll),
  // the traces last / max_hold / min_hold (3 x vw_w floats), the pending group's accumulator
  // (vw_w floats, or float64 linear sums for MEAN) and the scratch of a push's partials.  The
  // counters are host side: pushes are in call order
  int vw_h = 0, vw_w = 0, vw_c0 = 0, vw_c1 = 0, vw_det = 0, vw_m = 1, vw_scroll = 1;
  int64_t vw_off = 0;
  uint64_t vw_rows = 0, vw_lines = 0;
  int vw_pending = 0;
  int vw_kind = 0;                 // ViewForm::kind of the last push (test hook zfft__plan_view_form)
  DevBuf vw_ring, vw_img, vw_tr, vw_pend, vw_scratch, vw_rgba;
  // row history (zfft_plan_history; zfft_history.cpp): hs_cap = 0 is off (no buffer).  hs_store
  // holds hs_cap slots of hs_stride elements in hs_q.format, row R in slot R mod hs_cap; hs_seen
  // counts the rows pushed (host side: pushes are in call order).  hs_img / hs_rgba are a host
  // view's image and pixels, hs_scratch a sliced view's partials, hs_replay the float rows of
  // zfft_history_replay_viewport; zfft_history_read stages its rows in row_stage
  int64_t hs_cap = 0, hs_stride = 0;
  zfft::HistQuant hs_q;
  uint64_t hs_seen = 0;
  int hs_kind = 0;                 // HistForm::kind of the last view (test hook zfft__plan_history_form)
  DevBuf hs_store, hs_img, hs_rgba, hs_scratch, hs_replay;
  // channel taps (zfft_plan_taps; zfft_tap.cpp): null = off (nothing allocated); the state is that file's
  zfft::TapState *tap = nullptr;
  // channeliser (zfft_plan_chan; zfft_chan.cpp): null = off (nothing allocated); the state is that file's
  zfft::ChanState *chan = nullptr;
  // demodulator bank (zfft_plan_demod; zfft_demod.cpp): null = off (nothing allocated); the state is that file's
  zfft::DemodState *demod = nullptr;
  // resampler bank (zfft_plan_resamp; zfft_resamp.cpp): null = off (nothing allocated); the state is that file's
  zfft::ResampState *resamp = nullptr;
  // level bank (zfft_plan_level; zfft_level.cpp): null = off (nothing allocated); the state is that file's
  zfft::LevelState *level = nullptr;
  // Ordering across streams: every call that enqueues work first makes its stream wait for
  // the plan's previous work (done_ev, recorded on done_st), then records done_ev after its
  // own; the workspaces, tables and the ring are thus used in call order whatever streams the
  // caller picks, and a synchronous table upload waits for done_ev first.
  hipEvent_t done_ev = nullptr;
  hipStream_t done_st = nullptr;
  bool has_work = false;
  // (the walk's and FC's frame-end maps follow the decimator on its own stream and keep V^T x in
  // LDS: no stream, event or buffer of theirs here)
  // FC decimator (paths 6, 7): W_M twiddles (M = 8192 / the head's zoom), then one C row per LO frequency; fc_built holds the
  // f_lo / fs ratios the rows were built for (rebuilt when they change; empty: not built)
  DevBuf fc_tab;
  std::vector<double> fc_built;
  // FC tails of zoom >= 16 (path 7): per launch zoom 8, 4, 2 the twiddles W_M^k and one row at
  // f_lo = 0 for the unit LO table, one after another; uploaded once
  DevBuf fc_tail_tab;
};

namespace zfft {

// --- zfft_plan.cpp ---
int fail(int code, const std::string &msg);  // sets the thread's error message, returns code
int hip_fail(hipError_t e, const char *where);
// Timing marks: an event before the first launch and after each launch (or launch group)
// of a call, with the name of what ran since the previous mark.
void mark(zfft_plan *p, hipStream_t st, const char *what = "");
// Order `st` after everything the plan enqueued before (on any stream).
int use_stream(zfft_plan *p, hipStream_t st);
// Opens a device call on the caller's stream handle: *st = that stream, ordered after the plan's
// earlier work (use_stream), the timing marks restarted with "start" on it.
int begin_call(zfft_plan *p, void *hip_stream, hipStream_t *st);
// Mark the end of the plan's work enqueued so far on `st`.
int done_on(zfft_plan *p, hipStream_t st);
// Wait on the host until the plan's enqueued work is done (before a synchronous upload
// overwrites a table that work may still read).
int quiesce(zfft_plan *p);
int enter(zfft_plan *p);  // null check + hipSetDevice
// Grows a buffer an enqueued call may still use: nothing when it holds `bytes`, else quiesce, then
// a new allocation; ZFFT_ENOMEM "<what> allocation failed" (HIP's sticky error cleared).
int grow(zfft_plan *p, DevBuf &b, size_t bytes, const char *what);
// Ends a synchronous read: given the status of the copies enqueued on the plan's stream, marks the
// plan's work done there and waits for it; a failure is ZFFT_EHIP "<what>: ...".
int sync_read(zfft_plan *p, hipError_t e, const char *what);
// `count` host rows of n_win floats into the plan's one device staging row_stage (grown under
// `what`), copied on the plan's stream after the plan's earlier work; *d_rows = the staging.
// Every row consumer shares the buffer, and zfft_history_read uses it for the other direction.
// That is safe only while every user copies and launches on p->stream and waits for that stream
// before it returns: a new user must do the same, or take a buffer of its own.
int stage_rows(zfft_plan *p, const float *rows, int32_t count, const char *what, const float **d_rows);
// `bytes` of host rows into the page-locked row_pin, which the display kernels read in place;
// *d_rows = its device address.  A growth waits for the plan's work before it frees.  The callers
// wait for their kernels before they return: no kernel still reads row_pin at the next call.
int pin_rows(zfft_plan *p, const float *rows, size_t bytes, const float **d_rows);
// Rows per call: int row indices; the detector's count * max_per_row records stay below 2^31.
constexpr int32_t kMaxPushRows = 1 << 30, kMaxDetectRows = 1 << 26;
// Real input at zoom 1 takes scipy.signal.welch's one-sided branch.
inline bool onesided(const zfft_plan *p) { return p->cfg.in_dtype == kInF32R && p->K == 0; }
int row_length(const zfft_plan *p);  // valid entries per row
// Rows per frame of L input samples (zfft_plan_segments_per_line): 1 unless 1 <= g < nseg.
int64_t lines_per_frame(const zfft_plan *p, int64_t L);
// A NULL stream handle means HIP's default (null) stream, as everywhere in HIP.
inline hipStream_t pick_stream(zfft_plan *, void *s) { return (hipStream_t)s; }

// --- zfft_waterfall.cpp ---
// The colormap LUT on the device (built and uploaded on first use, on st) and makeARGB's levels
// as waterfall_render_kernel takes them; needs no ring.
int render_setup(zfft_plan *p, hipStream_t st, double *lo, double *scale);
// An image up to this size is written straight into a page-locked host destination by the
// kernel; a larger one goes through a device buffer and one copy.
constexpr size_t kDisplayZeroCopyMax = (size_t)4 << 20;

// --- zfft_decim.cpp ---
// Stage lengths: n_0 = L, n_{k+1} = ceil(n_k / 2)  (decimate(...)[::2]).
std::vector<int64_t> stage_lengths(int64_t L, int K);
int ensure_lo(zfft_plan *p, int64_t L);
// The plan's K stages on `frames` frames of L samples (n = stage_lengths(L, K)), by the
// schedule choose_schedule gives; *out = the decimated frames, natural layout.
int run_decimator(zfft_plan *p, const InDesc &in, int64_t L, int frames,
                  const std::vector<int64_t> &n, const float2 **out, hipStream_t st);

// --- zfft_track.cpp ---
// Frees the emission tracker and switches it off (the caller has waited for the plan's work).
void track_release(zfft_plan *p);
// Everything of the tracker back to zero, in stream order; nothing while it is off.
int track_restart(zfft_plan *p);

// --- zfft_tap.cpp ---
// Frees the channel taps and switches them off (the caller has waited for the plan's work).
void tap_release(zfft_plan *p);

// --- zfft_chan.cpp ---
// Frees the channeliser and switches it off (the caller has waited for the plan's work).
void chan_release(zfft_plan *p);

// --- zfft_demod.cpp ---
// Frees the demodulator bank and switches it off (the caller has waited for the plan's work).
void demod_release(zfft_plan *p);

// --- zfft_resamp.cpp ---
// Frees the resampler bank and switches it off (the caller has waited for the plan's work).
void resamp_release(zfft_plan *p);

// --- zfft_level.cpp ---
// Frees the level bank and switches it off (the caller has waited for the plan's work).
void level_release(zfft_plan *p);

// --- zfft_welch.cpp ---
// The Welch rows (or lines) of `frames` decimated frames of Ld samples at x into d_rows, by the
// form choose_welch gives; builds the window tables on first use.
int run_welch(zfft_plan *p, const float2 *x, int64_t Ld, int frames, float *d_rows, hipStream_t st);

}  // namespace zfft
