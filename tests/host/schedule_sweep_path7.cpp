// schedule_sweep_path7.cpp -- stand-alone sweep of choose_schedule (csrc/zfft_schedule.cpp) on
// path 7 (FC wherever a form exists) over the domain tests/host/schedule_sweep.cpp sweeps for
// paths 0 .. 6, built with ASan + UBSan by tests/test_schedule_path7.py: FC heads and FC tails
// only inside FC's domain, path 7 equal to path 6 wherever it adds no form, and no 64-bit
// product overflows (UBSan would stop the program).  No HIP, no plan.
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
  long n = 0, fc2 = 0, fct = 0;
  for (int K = 0; K <= 9; ++K)
    for (int elem : elems)
      for (int64_t L : Ls)
        for (int frames : Fs) {
          const SchedKey k{K, elem, 7, L, frames}, k6{K, elem, 6, L, frames};
          const Schedule s = choose_schedule(k), s6 = choose_schedule(k6);
          ++n;
          const char *name = schedule_name(s);
          check(name && std::strlen(name) > 0 && std::strlen(name) < 32, "name", k, s);
          check(s.rc == ZFFT_OK || s.rc == ZFFT_EUNSUPPORTED, "rc value", k, s);
          check((s.rc == ZFFT_OK) == (s.why == nullptr), "a message exactly when refused", k, s);
          check(s.rc == s6.rc, "refused exactly where path 6 is", k, s);
          (void)batches_keep_xa(k);
          if (s.rc != ZFFT_OK) continue;
          const bool fits = L >= 16384 && L * (int64_t)elem < two31 && frames <= 65535;
          const bool fch = s.head == Head::Fc2 || s.head == Head::Fc4 || s.head == Head::Fc8;
          const bool pc = fch || s.head == Head::Pc2Tiles || s.head == Head::Pc4Tiles ||
                          s.head == Head::Pc8Tiles || s.head == Head::Walk4 || s.head == Head::Walk8;
          check(!fch || fits, "FC head: 16384 <= L, frame < 2^31 bytes, frames <= 65535", k, s);
          check(!pc || (L >= 16384 && frames <= 65535), "PC: L >= 16384, frames <= 65535", k, s);
          check(K == 0 || pc, "path 7 runs a PC / FC form or is refused", k, s);
          // where FC has a form and the frame fits, path 7 takes it
          check(!(K == 1 && fits) || s.head == Head::Fc2, "zoom 2 in FC's domain: fc2", k, s);
          check((s.head == Head::Fc2) == (K == 1 && fits), "fc2 only at zoom 2", k, s);
          check(!(K >= 2 && fits) || s.head == (K == 2 ? Head::Fc4 : Head::Fc8), "zoom >= 4 in FC's domain", k, s);
          // the FC tail: after an FC head, on its complex64 output of ceil(L / 8) samples
          const int64_t n3 = (L + 7) / 8;
          if (s.tail == Tail::Fc) {
            ++fct;
            check(K > 3 && s.head == Head::Fc8 && s.head_stages == 3, "FC tail: zoom >= 16 after fc8", k, s);
            check(n3 >= 16384 && n3 * 8 < two31, "FC tail: 16384 <= input, < 2^31 bytes", k, s);
          } else {
            check(!(K > 3 && s.head == Head::Fc8 && n3 >= 16384), "FC tail wherever its first launch fits", k, s);
          }
          check(s.head_stages >= 0 && s.head_stages <= K, "head_stages <= K", k, s);
          check(s.tail == Tail::None ? (s.head_stages == K) : (K > 3 && s.head_stages == 3),
                "a tail only at zoom >= 16, after three stages", k, s);
          if (s.tail == Tail::Xa) check(n3 * 8 < two31, "XA tail: stage arrays < 2^31 bytes", k, s);
          // everything else is path 6's answer
          if (s.head != Head::Fc2 && s.tail != Tail::Fc)
            check(s.head == s6.head && s.tail == s6.tail && s.head_stages == s6.head_stages, "else as path 6", k, s);
          if (s.tail == Tail::Fc) check(s.head == s6.head && s.head_stages == s6.head_stages, "path 6's head", k, s);
          fc2 += s.head == Head::Fc2;
        }
  if (!fc2 || !fct) {
    std::printf("schedule_sweep_path7: no fc2 (%ld) or no FC tail (%ld) in the sweep\n", fc2, fct);
    return 1;
  }
  if (g_bad) {
    std::printf("schedule_sweep_path7: %d of %ld keys failed\n", g_bad, n);
    return 1;
  }
  std::printf("schedule_sweep_path7: ok (%ld keys, %ld fc2, %ld FC tails)\n", n, fc2, fct);
  return 0;
}
