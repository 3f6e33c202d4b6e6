// schedule_sweep.cpp -- stand-alone sweep of choose_schedule (csrc/zfft_schedule.cpp) over its
// whole domain, built with ASan + UBSan by tests/test_schedule.py: the domain limits of every
// kernel form hold for whatever the chooser returns, and its 64-bit products do not overflow
// (UBSan would stop the program).  No HIP, no plan.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "zfft.h"
#include "zfft_schedule.h"

using namespace zfft;

static int g_bad = 0;
static void check(bool ok, const char *what, const SchedKey &k, const Schedule &s) {
  if (ok) return;
  if (++g_bad <= 20)
    std::printf("FAIL %s: K=%d elem=%d path=%d L=%lld frames=%d -> rc=%d %s\n", what, k.K, k.elem_bytes,
                k.path, (long long)k.L, k.frames, s.rc, schedule_name(s));
}

int main() {
  const int64_t two31 = (int64_t)1 << 31;
  const int elems[] = {8, 4, 2, 4};  // complex64, complex32, cu8, real f32
  const int64_t Ls[] = {28, 8191, 8192, 16383, 16384, (int64_t)1 << 19, ((int64_t)1 << 19) + 1,
                        ((int64_t)1 << 28) - 1, (int64_t)1 << 28, (int64_t)1 << 30};
  const int Fs[] = {1, 15, 16, 31, 32, 383, 384, 511, 512, 767, 768, 1023, 1024, 65535, 65536, INT32_MAX};
  long n = 0;
  for (int K = 0; K <= 9; ++K)
    for (int elem : elems)
      for (int path = 0; path <= 6; ++path)
        for (int64_t L : Ls)
          for (int frames : Fs) {
            const SchedKey k{K, elem, path, L, frames};
            const Schedule s = choose_schedule(k);
            ++n;
            const char *name = schedule_name(s);
            check(name && std::strlen(name) > 0 && std::strlen(name) < 32, "name", k, s);
            check(s.rc == ZFFT_OK || s.rc == ZFFT_EUNSUPPORTED, "rc value", k, s);
            check(s.rc == ZFFT_OK || path >= 3, "refused only on path >= 3", k, s);
            check((s.rc == ZFFT_OK) == (s.why == nullptr), "a message exactly when refused", k, s);
            (void)xa_min_frames(L);
            (void)batches_keep_xa(k);
            if (s.rc != ZFFT_OK) continue;
            const bool fc = s.head == Head::Fc4 || s.head == Head::Fc8;
            const bool pc = fc || s.head == Head::Pc2Tiles || s.head == Head::Pc4Tiles ||
                            s.head == Head::Pc8Tiles || s.head == Head::Walk4 || s.head == Head::Walk8;
            const bool in32 = L * 8 < two31 && L * (int64_t)elem < two31;
            check(!fc || (L >= 8192 && L * (int64_t)elem < two31), "FC: L >= 8192, frame < 2^31 bytes", k, s);
            check(s.head != Head::Xa || in32, "XA head: stage arrays < 2^31 bytes", k, s);
            // The XA tail reads the head's complex64 output, ceil(L / 8) samples per frame.  On the
            // automatic path the head itself is taken only where XA fits the input frame; a forced
            // path 4 / 5 / 6 takes the head whatever the frame's size (as it always has), so there
            // the tail's own arrays are what must fit.
            if (s.tail == Tail::Xa)
              check(path == 0 ? in32 : ((L + 7) / 8) * 8 < two31, "XA tail: stage arrays < 2^31 bytes", k, s);
            check(!pc || (L >= 16384 && frames <= 65535), "PC: L >= 16384, frames <= 65535", k, s);
            check(s.head_stages >= 0 && s.head_stages <= K, "head_stages <= K", k, s);
            check(s.tail == Tail::None ? (s.head_stages == K) : (K > 3 && s.head_stages == 3),
                  "a tail only at zoom >= 16, after three stages", k, s);
            check((path != 1 && path != 2) || s.head == Head::Exact || s.head == Head::Fused,
                  "paths 1, 2: exact or fused only", k, s);
            check(path != 1 || s.head == Head::Exact, "path 1: exact", k, s);
            check(path != 3 || s.head == Head::Xa || K == 0, "path 3: XA", k, s);
          }
  if (g_bad) {
    std::printf("schedule_sweep: %d of %ld keys failed\n", g_bad, n);
    return 1;
  }
  std::printf("schedule_sweep: ok (%ld keys)\n", n);
  return 0;
}
