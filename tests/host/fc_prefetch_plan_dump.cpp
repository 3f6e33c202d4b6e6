// Prints the FC decimator's prefetch group plans (pypanadapter_amd/csrc/fc_prefetch_plan.h, the
// header fc_kernels.hip is compiled from) for tests/test_fc_prefetch_plan.py, one line per
// instantiation and group:
//   Z DT FLIP S KEEP point  pair pair ...     (pair: index among a thread's 16 pairs of a window)
// Plain g++, no HIP.
#include <cstdio>

#include "fc_prefetch_plan.h"

using namespace zfft::fc;

int main() {
  const int zooms[] = {8, 4, 2}, dts[] = {kPfC64, kPfC32H, kPfCU8, kPfF32R};
  for (int Z : zooms)
    for (int DT : dts)
      for (int FLIP = 0; FLIP < 2; ++FLIP) {
        const int S = pf_step(Z), KEEP = 16 - S;
        for (int g = 0; g < kPfPoints; ++g) {
          std::printf("%d %d %d %d %d %d ", Z, DT, FLIP, S, KEEP, g);
          // as the kernel's pf_group: pf[i] = pair KEEP + i for i in [first, first + n)
          const int first = pf_first(Z, DT, FLIP, g), n = pf_count(Z, DT, FLIP, g);
          for (int i = first; i < first + n; ++i) std::printf(" %d", KEEP + i);
          std::printf("\n");
        }
      }
  return 0;
}
