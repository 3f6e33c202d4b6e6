// Stand-alone driver of zfft::median_bias (csrc/zfft_median_bias.h; no HIP, no Python): prints
// bias(n) for n = 1 .. argv[1] with 17 significant digits, one per line, for
// tests/test_welch_average.py to compare with scipy's _median_bias.
#include <cstdio>
#include <cstdlib>

#include "zfft_median_bias.h"

int main(int argc, char **argv) {
  const int nmax = argc > 1 ? std::atoi(argv[1]) : 300;
  if (nmax < 1 || nmax > 1000000) return 2;
  for (int n = 1; n <= nmax; ++n) std::printf("%d %.17g\n", n, zfft::median_bias(n));
  return 0;
}
