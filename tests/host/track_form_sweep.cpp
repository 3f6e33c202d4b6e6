// track_form_sweep.cpp -- stand-alone sweep of choose_track and the host side of the open table
// (csrc/zfft_track_plan.cpp) over their domain, built with ASan + UBSan by
// tests/test_track_host.py: every (K, gap, count) gets a form whose chunks fit the labelling
// kernel's LDS and whose passes fit the scratch and cover the call; outside the domain it
// refuses; track_open_records sorts, filters and cuts a full frontier.  No HIP, no plan.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "zfft_track_plan.h"

using namespace zfft;

static long g_bad = 0;
static void check(bool ok, const char *what, int K, int gap, int count) {
  if (ok) return;
  if (++g_bad <= 20) std::printf("FAIL %s: K=%d gap=%d count=%d\n", what, K, gap, count);
}

int main() {
  const int counts[] = {1,    2,    7,     8,     9,     15,    16,     17,      63,      64,      65,     4095,
                        4096, 4097, 8191,  8192,  8193,  16383, 16384,  16385,   32759,   32760,   32761,  69632,
                        131063, 131064, 131065, 1 << 20, (1 << 20) + 1, 1 << 26};
  long n = 0;
  for (int K = 1; K <= kTrackMaxK; ++K)
    for (int gap = 0; gap <= kTrackMaxGap; ++gap)
      for (int count : counts) {
        const TrackForm f = choose_track(K, gap, count);
        ++n;
        check(f.ok(), "a form for every call", K, gap, count);
        if (!f.ok()) continue;
        const int G = gap + 1;
        check(f.chunk_rows == 16 || f.chunk_rows == 32 || f.chunk_rows == 64, "16, 32 or 64 rows per chunk", K, gap, count);
        check(f.chunk_rows >= G, "a chunk is no shorter than the look-back", K, gap, count);
        check(f.chunk_rows * K <= kTrackChunkNodes, "a chunk's runs fit the LDS arrays", K, gap, count);
        check(f.pass_rows >= f.chunk_rows && f.pass_rows % f.chunk_rows == 0, "a pass is whole chunks", K, gap, count);
        check(((int64_t)f.pass_rows + G) * K <= kTrackPassNodes, "a pass's nodes fit the scratch", K, gap, count);
        check((int64_t)f.passes * f.pass_rows >= count && (int64_t)(f.passes - 1) * f.pass_rows < count,
              "the passes cover the call, none empty", K, gap, count);
        const int first = count < f.pass_rows ? count : f.pass_rows;
        check(f.chunks == f.chunks_of(first) && (int64_t)f.chunks * f.chunk_rows >= first &&
                  (int64_t)(f.chunks - 1) * f.chunk_rows < first,
              "the chunks cover the pass, none empty", K, gap, count);
        check(track_scratch_bytes(K, gap, first) == ((size_t)first + G) * K * 76 + ((size_t)first + G) * 8,
              "the scratch is 76 bytes a node and 8 a row", K, gap, count);
        check(count < 64 * 256 || f.chunk_rows == 64, "a long call takes 64-row chunks", K, gap, count);
      }
  check(choose_track(8, 0, 69632).passes == 1, "cfg2's step is one pass", 8, 0, 69632);
  for (int K : {0, -1, 33, INT32_MAX, INT32_MIN}) check(!choose_track(K, 0, 5).ok(), "refused K", K, 0, 5);
  for (int gap : {-1, 8, INT32_MAX, INT32_MIN}) check(!choose_track(8, gap, 5).ok(), "refused gap", 8, gap, 5);
  for (int count : {0, -1, (1 << 26) + 1, INT32_MAX, INT32_MIN})
    check(!choose_track(8, 0, count).ok(), "refused count", 8, 0, count);

  // the open table: a full frontier of 8 rows x 32 slots, every run a track of its own, names
  // descending with the index; then the same with half the runs folded into their neighbour
  for (int K : {1, 8, 32})
    for (int G : {1, 3, 8})
      for (int fold = 0; fold < 2; ++fold) {
        const int nf = G * K;
        std::vector<int32_t> found(G, K);
        found[G - 1] = K + 5;  // clamped
        if (G > 1) found[0] = -3;  // none
        std::vector<uint32_t> parent(nf);
        std::vector<TrackOpen> tab(nf);
        int want = 0;
        for (int i = 0; i < nf; ++i) {
          parent[i] = fold && (i % 2) ? (uint32_t)(i - 1) : (uint32_t)i;
          std::memset(&tab[i], 0, sizeof(TrackOpen));
          tab[i].name = (uint64_t)(1000 - i) * 32 + (uint64_t)(i % K);
          tab[i].row_last = 2000 + i;
          tab[i].peak_key = 0x3D59FFFFu;  // det_key(-83.0f): ~0xC2A60000
          const bool used = !(G > 1 && i / K == 0);
          if (used && parent[i] == (uint32_t)i) ++want;
        }
        for (int max : {0, 1, want - 1, want, want + 7, kTrackFrontier}) {
          if (max < 0) continue;
          std::vector<zfft_track> out((size_t)max + 1);
          std::memset(out.data(), 0x5a, out.size() * sizeof(zfft_track));
          const int got = track_open_records(found.data(), parent.data(), tab.data(), K, G, out.data(), max);
          check(got == (max < want ? max : want), "the number of open tracks, cut at max", K, G, max);
          for (int i = 0; i < got; ++i) {
            check(i == 0 || out[i - 1].row_first < out[i].row_first ||
                      (out[i - 1].row_first == out[i].row_first && out[i - 1].slot_first < out[i].slot_first),
                  "ascending names", K, G, i);
            check(out[i].peak_db == -83.0f && out[i].reserved == 0 && out[i].row_last - 2000 == 1000 - out[i].row_first,
                  "the record of its entry", K, G, i);
          }
          check(out[(size_t)max].reserved == 0x5a5a5a5a, "nothing beyond max", K, G, max);
          ++n;
        }
      }
  if (g_bad) {
    std::printf("track_form_sweep: %ld checks failed over %ld keys\n", g_bad, n);
    return 1;
  }
  std::printf("track_form_sweep: ok (%ld keys)\n", n);
  return 0;
}
