// zfft_track_plan.cpp -- choose_track and the host side of the open table (zfft_track_plan.h):
// pure host code, built into libzfft.so and, stand-alone under ASan + UBSan, into
// tests/host/track_form_sweep.cpp.
#include "zfft_track_plan.h"

#include <algorithm>
#include <cstring>

namespace zfft {

TrackForm choose_track(int K, int gap, int count) {
  TrackForm f;
  if (K < 1 || K > kTrackMaxK || gap < 0 || gap > kTrackMaxGap || count < 1 || count > (1 << 26)) return f;
  const int G = gap + 1;
  int c = 64;  // 64 * 32 slots = kTrackChunkNodes
  while (c > 16 && count < c * 256) c /= 2;
  f.chunk_rows = c;
  // a pass: as many whole chunks as kTrackPassNodes nodes hold beside the frontier's
  const int room = kTrackPassNodes / K - G;
  f.pass_rows = room / c * c;
  f.passes = (count + f.pass_rows - 1) / f.pass_rows;
  f.chunks = f.chunks_of(std::min(count, f.pass_rows));
  return f;
}

size_t track_scratch_bytes(int K, int gap, int rows) {
  const size_t lrows = (size_t)rows + (size_t)gap + 1, nodes = lrows * (size_t)K;
  return nodes * 76 + lrows * 8;
}

int track_open_records(const int32_t *fr_found, const uint32_t *fr_parent, const TrackOpen *tab, int K, int G,
                       zfft_track *out, int max) {
  int n = 0;
  TrackOpen tmp[kTrackFrontier];
  for (int i = 0; i < G * K && i < kTrackFrontier; ++i) {
    const int used = std::min(std::max(fr_found[i / K], 0), K);
    if (i % K < used && fr_parent[i] == (uint32_t)i) tmp[n++] = tab[i];
  }
  std::sort(tmp, tmp + n, [](const TrackOpen &a, const TrackOpen &b) { return a.name < b.name; });
  const int m = std::min(n, std::max(max, 0));
  for (int i = 0; i < m; ++i) out[i] = track_record(tmp[i]);
  return m;
}

}  // namespace zfft

// Test hook (not part of include/zfft.h): {chunk_rows, pass_rows, passes, chunks} of a call.
extern "C" int zfft__track_form(int32_t K, int32_t gap, int32_t count, int32_t *out4) {
  const zfft::TrackForm f = zfft::choose_track(K, gap, count);
  if (!f.ok() || !out4) return -1;
  out4[0] = f.chunk_rows, out4[1] = f.pass_rows, out4[2] = f.passes, out4[3] = f.chunks;
  return 0;
}
