// The bias of the median of n chi-square(2) variates relative to their mean -- what
// scipy.signal.welch(average='median') divides its median by (scipy.signal._spectral_py
// _median_bias): 1 + sum_{i=1..(n-1)/2} (1/(2i+1) - 1/(2i)).  Pure host code (no HIP), so a
// stand-alone program can test it (tests/host/median_bias_main.cpp).
#pragma once

namespace zfft {

inline double median_bias(int n) {
  // -1 / (2i (2i+1)), smallest terms first, in extended precision: within an ulp of the exact
  // sum (scipy's pairwise numpy sum is no closer)
  long double sum = 0.0L;
  for (int i = (n - 1) / 2; i >= 1; --i) {
    const long double e = 2.0L * (long double)i;
    sum -= 1.0L / (e * (e + 1.0L));
  }
  return (double)(1.0L + sum);
}

}  // namespace zfft
