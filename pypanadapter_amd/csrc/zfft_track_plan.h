// zfft_track_plan.h -- how a push of the emission tracker (track_kernels.hip; rule in zfft.h,
// zfft_plan_track) is cut, as a value: a pure host function of the detector's K, the gap and the
// rows of the call.  No HIP, no plan: zfft_track.cpp launches what it returns and
// tests/test_track_host.py sweeps it without a device.
#pragma once

#include <cstddef>
#include <cstdint>

#include "zfft.h"  // zfft_track, zfft_emission

namespace zfft {

constexpr int kTrackMaxGap = 7;           // rows an emission may be absent for
constexpr int kTrackMaxSlack = 64;        // columns two linked runs may be apart
constexpr int kTrackMaxTracks = 1 << 22;  // the store's capacity, at most
constexpr int kTrackMaxK = 32;            // = kDetectMaxPerRow
constexpr int kTrackFrontier = (kTrackMaxGap + 1) * kTrackMaxK;  // 256 runs, 256 open tracks at most
constexpr int kTrackThreads = 256;        // threads of every workgroup but the scan's
constexpr int kTrackScanThreads = 1024;   // the one workgroup of track_scan
constexpr int kTrackChunkNodes = 2048;    // runs a chunk's workgroup labels in LDS, at most
constexpr int kTrackPassNodes = 1 << 20;  // runs of a pass (the frontier's included), at most

// A call's rows go through the kernels in passes of `pass_rows` rows (the scratch holds one pass;
// the state carried from pass to pass is the state carried from call to call), a pass in chunks
// of `chunk_rows` rows: one workgroup labels a chunk's runs in LDS, the links across a chunk's
// first row (a seam) are made by a second launch.  A node is a (row, slot) pair: the frontier's
// gap + 1 rows first, then the pass's rows, `K` slots each.
struct TrackForm {
  int chunk_rows = 0;  // rows per chunk: 16, 32 or 64, never below gap + 1
  int pass_rows = 0;   // rows per pass: a multiple of chunk_rows
  int passes = 0;      // passes of this call
  int chunks = 0;      // chunks of the first (largest) pass
  bool ok() const { return chunk_rows > 0; }
  // of a pass on `rows` rows
  int chunks_of(int rows) const { return (rows + chunk_rows - 1) / chunk_rows; }
};

// 64 rows per chunk where that still gives 256 workgroups, 32 and 16 below that (a short call
// spreads over more of the chip; a chunk never has fewer rows than the look-back gap + 1 = 8 at
// most); chunk_rows * K <= kTrackChunkNodes always.  !ok() outside 1 <= K <= 32, 0 <= gap <= 7,
// 1 <= count <= 2^26.
TrackForm choose_track(int K, int gap, int count);

// Bytes of the scratch of a pass on `rows` rows: per node the aggregates (56), the peak of a
// chunk's part (16) and the union-find parent (4), per row (the frontier's included) a count and
// an offset.
size_t track_scratch_bytes(int K, int gap, int rows);

// The tracker's record as the kernels carry it for an open track (the open table, one entry per
// frontier run that represents a track) -- plain values.
struct TrackOpen {
  uint64_t name;  // row_first * 32 + slot_first
  int64_t row_last, peak_row;
  uint64_t cells, runs;
  int32_t col_first, col_last, peak_col;
  uint32_t peak_key;  // det_key of peak_db with -0.0 taken as 0.0
};
static_assert(sizeof(TrackOpen) == 56, "TrackOpen is 56 bytes");

// The tracker's counters on the device (rows_seen is the host's: pushes are in call order).
struct TrackCounters {
  uint64_t unread, dropped, short_tracks, truncated_rows, open, pending;
};

#if defined(__HIPCC__)
#define ZFFT_TRACK_HD __host__ __device__
#else
#define ZFFT_TRACK_HD
#endif

// zfft_track of an entry (peak_key back to the float: zfft_detect_keys.h's map, inverted).
ZFFT_TRACK_HD inline zfft_track track_record(const TrackOpen &a) {
  zfft_track t;
  t.row_first = (int64_t)(a.name >> 5);
  t.row_last = a.row_last;
  t.peak_row = a.peak_row;
  t.cells = a.cells;
  t.runs = a.runs;
  t.col_first = a.col_first;
  t.col_last = a.col_last;
  t.peak_col = a.peak_col;
  t.slot_first = (int32_t)(a.name & 31);
  const uint32_t bits = (a.peak_key & 0x80000000u) ? (a.peak_key ^ 0x80000000u) : ~a.peak_key;
  union {
    uint32_t u;
    float f;
  } cv;
  cv.u = bits;
  t.peak_db = cv.f;
  t.reserved = 0;
  return t;
}

// The open tracks of a frontier copied to the host (fr_found: G rows, already within [0, K];
// fr_parent, tab: G * K entries), in ascending (row_first, slot_first): at most `max` records
// into out; returns their number.
int track_open_records(const int32_t *fr_found, const uint32_t *fr_parent, const TrackOpen *tab, int K, int G,
                       zfft_track *out, int max);

}  // namespace zfft
