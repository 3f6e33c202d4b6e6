// zfft_schedule.cpp -- the decimator schedule chooser (zfft_schedule.h): every measured
// crossover between the schedules and every domain limit of one, in one pure function.
#include "zfft_schedule.h"

#include <cstddef>  // (zfft.h uses size_t)

#include "zfft.h"

namespace zfft {
namespace {

// Auto choice between XA (one wave per frame) and the blocked schedules, from the sweep
// tools/sweep_schedule.py (profiles/r03i/sweep_schedule.json: ms per call, N = 4096, zoom 8):
// XA needs enough frames to fill 2 waves x 1024 SIMDs; for ~300k-sample frames it is the
// fastest from 384 frames (1.66 ms against 1.80 fused / 1.83 exact; 256 frames: 1.62 against
// 1.25 exact), for 2^20-sample frames from 768 (5.67 against 7.69 fused; 512: 5.56 against 5.28).
constexpr int kXaMinFrames = 768;
constexpr int kXaMinFramesShort = 384;
constexpr int64_t kXaShortFrame = (int64_t)1 << 19;
bool auto_xa(int frames, int64_t L) { return frames >= xa_min_frames(L); }

// XA addresses a frame's stage input and output through 32-bit buffer resources (stage
// outputs are complex64: 8 bytes per sample).
bool xa_fits(const SchedKey &k) {
  return k.L * (int64_t)k.elem_bytes < ((int64_t)1 << 31) && k.L * 8 < ((int64_t)1 << 31);
}

// The fused blocked schedule (path 2) saves passes over the frame interior but adds the
// exact edge-window runs, whose launches cost about as much as a whole pass over a few
// frames: it wins only for large batches.  Same sweep (frames x samples, ms, path 1 / path 2):
// 2^20-sample frames 64: 1.15 / 1.33, 128: 2.20 / 2.04, 256: 4.04 / 3.30; ~300k-sample frames
// 256: 1.25 / 1.43 (and from 384 frames XA beats both).
constexpr int64_t kFusedMinSamples = (int64_t)1 << 27;  // per call
bool use_fused(const SchedKey &k) {
  if (k.path == 1 || k.K < 2) return false;
  if (8 * edge_window(k.K) > k.L) return false;  // windows cost <= 1/4 of a frame
  return k.path == 2 || (int64_t)k.frames * k.L >= kFusedMinSamples;
}

// KW (one workgroup per frame) from this many frames per call; below, K1 + K2's tiles.
// tools/sweep_walk.py (profiles/r06k/sweep_walk.json, round 6's walk; ms per call, tiles / walk):
// 299,008-sample frames 512: 0.78 / 0.78, 768: 1.08 / 1.12, 1024: 1.44 / 1.43, 2048: 2.64 /
// 2.53, 4096: 5.21 / 4.87; 2^20-sample frames 768: 3.34 / 3.44, 1024: 4.40 / 4.36, 2048: 8.54 /
// 8.27 (cfg5), 4096: 16.8 / 16.0.  One workgroup per frame needs about two rounds of the chip's
// 512 resident workgroups to fill it; KW also keeps y2 (2 B per input sample) off HBM.  (Round
// 4 measured the walk level with the tiles up to 4096 frames: the threshold was 4096.)
constexpr int kPcWalkMinFrames = 1024;
// Zoom 4: the two-stage walk from this many frames per call, the tiles below; XA no longer
// wins anywhere PC fits (cfg1's 262,144-sample frames, ms per call, XA / tiles / walk: 256:
// 1.24 / 0.47 / 0.50, 512: 1.32 / 0.90 / 0.78, 1024: 1.69 / 1.69 / 1.44, 4096 (cfg1): 5.17 /
// 6.27 / 4.89; profiles/r06k/sweep_walk.json).
constexpr int kPc4WalkMinFrames = 512;
// Zoom 8 (and the zoom >= 16 head): FC (path 6, fc_kernels.hip) from this many frames per call,
// PC's tiles below.  ms per call, tiles / walk / FC (tools/fc_ab.py, profiles/r06fc3/fc_ab.json):
// 299,008-sample frames 1: 0.053 / 0.39 / 0.064, 16: 0.078 / 0.41 / 0.078, 64: 0.124 / 0.41 /
// 0.107, 512: 0.75 / 0.74 / 0.52, 4096: - / 4.69 / 3.44; 2^20-sample frames 1: 0.057 / 1.23 /
// 0.066, 64: 0.37 / 1.30 / 0.26, 2048: - / 9.05 / 6.61.
constexpr int kFcMinFrames = 16;
// Zoom 4 (cfg1's 262,144-sample frames, ms per call, tiles / walk / FC, profiles/r06fc/r06fc8):
// 1: 0.055 / 0.39 / 0.062, 16: 0.080 / 0.41 / 0.083, 64: 0.146 / 0.43 / 0.129, 512: 0.93 / 0.80 /
// 0.61, 4096: - / 5.06 / 3.77.
constexpr int kFc4MinFrames = 32;
// FC takes frames of >= 8192 samples (its window) below 2^31 bytes (its buffer loads' 32-bit
// offsets).
bool fc_fits(const SchedKey &k) {
  return k.L >= kSchedFcMinL && k.L * (int64_t)k.elem_bytes < ((int64_t)1 << 31);
}
// Every PC form: frames of >= kPcMinL samples, grid y = frames.
bool pc_any_fits(const SchedKey &k) { return k.L >= kPcMinL && k.frames <= 65535; }
// Zoom 8: the PC polyphase cascade.
bool pc_fits(const SchedKey &k) { return k.K == kSchedPcStages && pc_any_fits(k); }
// Zoom 4 (two stages): the walk (pc_walk_kernel<4>, path 5, automatic from kPc4WalkMinFrames:
// round 5's form lost to XA at cfg1, 4.49 against 4.34 ms, profiles/r05h; round 6's walk wins)
// and the tiles (K1 = FIR alpha into y1, K2 = the zoom-8 tail kernel on zoom 4's tables: path 4,
// automatic below the walk's batch).
bool pc4_fits(const SchedKey &k) { return k.K == 2 && pc_any_fits(k); }
// Zoom-4 tiles against XA (cfg1's 262,144-sample frames, profiles/r05u, ms per call): 1 frame
// 0.061 / 1.14 (blocked passes 0.22), 64: 0.14 / 1.21 (0.28), 256: 0.46 / 1.24, 384: 0.65 /
// 1.26 -- XA, one wave per frame, needs about a thousand frames to fill the chip; from 512
// frames the zoom-4 walk beats both (kPc4WalkMinFrames).
// Zoom 2 (one stage): the tail kernel on the mixed input in XA's factorisation (D forward at
// the input rate, the 25-tap FIR M, D2 backward at half rate), automatic below
// 512 frames per call: cfg2's 299,008-sample frames, ms per call, tiles / XA (profiles/r05y):
// 1 frame 0.048 / 0.89 (blocked passes 0.16), 64: 0.16 / 0.95 (0.28), 384: 0.85 / 1.18,
// 1024: 2.05 / 1.53 -- equal near 640.
constexpr int kPc2TilesMaxFrames = 512;
bool pc2_fits(const SchedKey &k) { return k.K == 1 && pc_any_fits(k); }
// Zoom >= 16: PC takes the first three stages (decimate x 3 exactly, frame-end maps included)
// and XA the remaining K - 3 on its 1/8-rate output -- the reference's stages are applied one
// after another (S:2096-2098), so the composition is the same cascade.
bool pc_head_fits(const SchedKey &k) { return k.K > kSchedPcStages && pc_any_fits(k); }

constexpr Schedule ok(Head h, int stages, Tail t = Tail::None) { return {ZFFT_OK, h, stages, t, nullptr}; }
constexpr Schedule refused(const char *why) { return {ZFFT_EUNSUPPORTED, Head::Exact, 0, Tail::None, why}; }

// Zoom 8's three stages (all of zoom 8, or the head of zoom >= 16).  PC (tiles below
// kFcMinFrames frames per call, FC from there) is the fastest schedule wherever it applies,
// from one frame per call (the reference's use: 0.053 against 0.37 ms for path 1) to full
// batches (4096 frames: FC 3.44 against the walk's 4.69 ms) -- tools/sweep_schedule.py,
// profiles/r04l; tools/fc_ab.py, profiles/r06fc3.  FC in the walk's place on request (6, 7) and
// automatic from kFcMinFrames; a forced 6 or 7 outside FC's domain runs the walk.
Head pc8_form(const SchedKey &k) {
  if (fc_fits(k) && (k.path >= 6 || (k.path == 0 && k.frames >= kFcMinFrames))) return Head::Fc8;
  if (k.path >= 5 || (k.path == 0 && k.frames >= kPcWalkMinFrames)) return Head::Walk8;
  return Head::Pc8Tiles;
}

}  // namespace

int xa_min_frames(int64_t L) { return L <= kXaShortFrame ? kXaMinFramesShort : kXaMinFrames; }

Schedule choose_schedule(const SchedKey &k) {
  if (k.K < 1) return ok(Head::Exact, 0);  // zoom 1: nothing to decimate
  if (k.path == 3 && !xa_fits(k))
    return refused("XA tiles (path 3) address a frame's stage arrays with 32-bit "
                   "offsets: frames of >= 2^31 bytes need path 0, 1 or 2");
  // exact tiles run one wave per frame: the schedule for batches that fill the GPU; the
  // blocked schedules split each frame over many waves and win for a few frames per call
  const bool pc_path = k.path == 0 || k.path >= 4;  // paths 1, 2, 3 never take PC
  if (k.path >= 4 && !pc_any_fits(k))
    return refused("PC decimator needs frames of >= 16384 samples and <= 65535 "
                   "frames per call");
  // the tiles hand a batch over to XA only where XA takes it (auto_xa: from 768 frames of
  // > 2^19 samples), never to the blocked passes, which lose to the tiles at every batch
  const bool xa_auto = auto_xa(k.frames, k.L) && xa_fits(k);
  // zoom 2: FC on request (path 7) where it fits; the tiles on request (paths 4, 5, 6; 7 outside
  // FC's domain) and automatic below 512 frames per call
  if (pc2_fits(k) && k.path == 7 && fc_fits(k)) return ok(Head::Fc2, 1);
  if (pc2_fits(k) && (k.path >= 4 || (k.path == 0 && (k.frames < kPc2TilesMaxFrames || !xa_auto))))
    return ok(Head::Pc2Tiles, 1);
  // zoom 4: the tiles below 32 frames per call, FC from there (the walk from 512 where FC
  // does not fit); all on request too
  if (pc4_fits(k) && pc_path) {
    if (fc_fits(k) && (k.path >= 6 || (k.path == 0 && k.frames >= kFc4MinFrames))) return ok(Head::Fc4, 2);
    if (k.path >= 5 || (k.path == 0 && k.frames >= kPc4WalkMinFrames)) return ok(Head::Walk4, 2);
    return ok(Head::Pc4Tiles, 2);
  }
  if (pc_fits(k) && pc_path) return ok(pc8_form(k), kSchedPcStages);
  // zoom >= 16: the head, then XA or zoom 2's tiles and the blocked passes for the rest (by the
  // tail's batch): XA where it takes the batch, except where zoom 2's tiles still beat it
  // (< 512 frames)
  if (pc_head_fits(k) && (k.path >= 4 || (k.path == 0 && xa_fits(k)))) {
    const int64_t n3 = (k.L + 7) >> kSchedPcStages;  // the head's output length
    const bool xa_tail = auto_xa(k.frames, n3) && !(k.frames < kPc2TilesMaxFrames && n3 >= kPcMinL);
    const Head head = pc8_form(k);
    // path 7: FC for the stages after an FC head too, while the head's output is long enough
    // for an FC launch (complex64 of n3 <= L / 8 samples: below 2^31 bytes wherever the head fits)
    if (k.path == 7 && head == Head::Fc8 && n3 >= kPcMinL) return ok(head, kSchedPcStages, Tail::Fc);
    return ok(head, kSchedPcStages, xa_tail ? Tail::Xa : Tail::Pc2TilesThenExact);
  }
  if (k.path == 3 || (k.path == 0 && xa_auto)) return ok(Head::Xa, k.K);
  if (use_fused(k)) return ok(Head::Fused, k.K);
  return ok(Head::Exact, k.K);
}

bool batches_keep_xa(const SchedKey &whole) {
  if (whole.path != 0 || !auto_xa(whole.frames, whole.L)) return false;
  const Schedule s = choose_schedule(whole);
  return s.rc == ZFFT_OK && (s.head == Head::Xa || s.tail != Tail::None);
}

const char *schedule_name(const Schedule &s) {
  if (s.rc != ZFFT_OK) return "unsupported";
  if (s.head_stages == 0) return "none";
#define ZFFT_SCHED_ROW(h) {h, h "+xa", h "+pc2_exact", h "+fc"}
  static const char *const names[11][4] = {
      ZFFT_SCHED_ROW("exact"),     ZFFT_SCHED_ROW("fused"),     ZFFT_SCHED_ROW("xa"),
      ZFFT_SCHED_ROW("pc2_tiles"), ZFFT_SCHED_ROW("pc4_tiles"), ZFFT_SCHED_ROW("pc8_tiles"),
      ZFFT_SCHED_ROW("walk4"),     ZFFT_SCHED_ROW("walk8"),     ZFFT_SCHED_ROW("fc4"),
      ZFFT_SCHED_ROW("fc8"),       ZFFT_SCHED_ROW("fc2")};
#undef ZFFT_SCHED_ROW
  return names[(int)s.head][(int)s.tail];
}

}  // namespace zfft
