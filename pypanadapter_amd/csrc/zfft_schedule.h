// zfft_schedule.h -- which decimator schedule a call takes, as a value: a pure host function
// of (stages, input element size, forced path, frame length, frames per call).  No HIP, no
// plan: zfft_decim.cpp launches what it returns, zfft_process sizes its batches by it and
// tests/test_schedule.py pins it without a device.
#pragma once

#include <cstdint>

namespace zfft {

struct SchedKey {
  int K;           // log2(zoom) decimation stages (0: zoom 1, no decimator)
  int elem_bytes;  // bytes per input sample (in_elem_bytes of the plan's in_dtype)
  int path;        // zfft_plan_path: 0 auto, 1 .. 7 forced
  int64_t L;       // samples per frame
  int frames;      // frames per call
};

// What runs the first stages (all K of them unless a tail follows).
enum class Head { Exact, Fused, Xa, Pc2Tiles, Pc4Tiles, Pc8Tiles, Walk4, Walk8, Fc4, Fc8, Fc2 };
// Zoom >= 16 after a three-stage PC / FC head: XA stages, or zoom 2's tiles while a stage's
// input has >= 16384 samples and the exact blocked passes after that, or (path 7) FC launches
// of three, two or one stages while a launch's input has >= 16384 samples and the former after
// that.
enum class Tail { None, Xa, Pc2TilesThenExact, Fc };

struct Schedule {
  int rc;           // ZFFT_OK or ZFFT_EUNSUPPORTED
  Head head;
  int head_stages;  // stages the head runs (K, or 3 as the head of zoom >= 16)
  Tail tail;
  const char *why;  // rc != ZFFT_OK: the error message (a string literal), else nullptr
};

// Constants of the choice that the runners' geometry shares.
constexpr int kSchedPcStages = 3;      // stages of the zoom-8 PC / FC forms (= kPcStages)
constexpr int64_t kSchedFcMinL = 8192;  // FC's window (= kFcN)
// PC decimator (pc_kernels.hip): frames long enough that the two frame ends' maps do not meet
constexpr int64_t kPcMinL = 16384;
// Fused schedule: edge width (final-stage samples) recomputed exactly, and the exact window length.
constexpr int kEdge = 384;
inline int64_t edge_window(int K) { return ((int64_t)1 << K) * (kEdge + 640); }

Schedule choose_schedule(const SchedKey &k);
// "fc8", "pc8_tiles+xa", "walk8+pc2_exact", "fc8+fc", ...; "none" at zoom 1, "unsupported" when refused
const char *schedule_name(const Schedule &s);

// Frames per call from which XA takes frames of L samples (where nothing faster applies).
int xa_min_frames(int64_t L);
// zfft_process batching: the whole call would go to XA (all stages, or the stages after the PC
// head of zoom >= 16), so each of its batches has to hold xa_min_frames(L) frames to keep it.
bool batches_keep_xa(const SchedKey &whole);

}  // namespace zfft
