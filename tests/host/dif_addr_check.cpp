// Walks the LDS slot rules of the in-place DIF Welch kernel (pypanadapter_amd/csrc/zfft_dif_addr.h,
// the header zfft_kernels.hip is compiled from) for tests/test_welch_dif_addr.py: for every size
// and every stage, every thread t and value k, the base-plus-constant address must be the slot of
// the element the stage means.  Prints one line per size and stage; a mismatch ends the run with
// its coordinates and status 1.  Then the window-hold table, one line per instantiation.
#include <cstdio>

#include "zfft_dif_addr.h"

namespace da = zfft::dif;

static int log2i(int n) {
  int l = 0;
  while ((1 << l) < n) ++l;
  return l;
}

int main() {
  for (int N = 1024; N <= 16384; N *= 2) {
    const int T = N / 16, P = log2i(N) / 4, R0 = N >> (4 * P), PM = R0 > 1 ? P : P - 1;
    // stage 1: element T k + t
    long checked = 0;
    for (int t = 0; t < T; ++t)
      for (int k = 0; k < 16; ++k, ++checked)
        if (da::slot(T * k + t) != da::slot(t) + da::slot_off(T, k) || da::slot_off(T, k) != (T + T / 16) * k) {
          std::printf("MISMATCH N=%d stage=1 t=%d k=%d\n", N, t, k);
          return 1;
        }
    const int k2 = da::second_base_from(T);
    for (int k = 0; k < 16; ++k) {
      const int off = k < k2 ? da::slot_off(T, k) : da::slot_off(T, k) - da::slot_off(T, k2);
      if (off < 0 || off > da::kMaxImmSlots) {
        std::printf("OFFSET N=%d stage=1 k=%d off=%d\n", N, k, off);
        return 1;
      }
    }
    std::printf("N=%d stage=1 stride=%d checked=%ld second_base_from=%d max_slot=%d\n", N, T, checked, k2,
                da::slot(T - 1) + da::slot_off(T, 15));
    // middle stages 2 .. PM: element base + S m, base = (t / S) 16 S + t mod S
    for (int st = 2; st <= PM; ++st) {
      const int S = N >> (4 * st);
      checked = 0;
      for (int t = 0; t < T; ++t) {
        const int base = da::mid_base(t, S);
        if (base != (t / S) * (16 * S) + t % S) {
          std::printf("BASE N=%d stage=%d t=%d\n", N, st, t);
          return 1;
        }
        for (int m = 0; m < 16; ++m, ++checked)
          if (da::slot(base + S * m) != da::slot(base) + da::slot_off(S, m) || da::slot_off(S, m) > da::kMaxImmSlots) {
            std::printf("MISMATCH N=%d stage=%d t=%d m=%d\n", N, st, t, m);
            return 1;
          }
      }
      std::printf("N=%d stage=%d stride=%d checked=%ld\n", N, st, S, checked);
    }
    // last stage: the thread's 16 consecutive slots
    for (int t = 0; t < T; ++t)
      for (int m = 0; m < 16; ++m)
        if (da::slot(16 * t + m) != da::slot(16 * t) + da::slot_off(1, m) || da::slot(16 * t) != 17 * t) {
          std::printf("MISMATCH N=%d last t=%d m=%d\n", N, t, m);
          return 1;
        }
    std::printf("N=%d last slots=%d\n", N, da::slot(N - 1) + 1);
  }
  for (int N = 1024; N <= 16384; N *= 2)
    for (int p = 0; p < 2; ++p)
      for (int h = 0; h < 2; ++h)
        for (int f = 0; f < 3; ++f)
          std::printf("hold %d %d %d %d %d  %d\n", N, p, h, f == 1, f == 2, da::win_hold(N, p, h, f == 1, f == 2));
  return 0;
}
