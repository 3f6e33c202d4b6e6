// detect_form_sweep.cpp -- stand-alone sweep of choose_detect (csrc/zfft_detect_plan.cpp) over
// its domain, built with ASan + UBSan by tests/test_detect_host.py: every row_len in [1, 65536]
// gets a form whose stated domain contains it, the narrowest of the forms the kernel file
// instantiates, with a grid the kernel's row loop covers; outside the domain it refuses.  No
// HIP, no plan.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "zfft_detect_plan.h"

using namespace zfft;

static long g_bad = 0;
static void check(bool ok, const char *what, int row_len, int count, const DetectForm &f) {
  if (ok) return;
  if (++g_bad <= 20)
    std::printf("FAIL %s: row_len=%d count=%d -> waves=%d per=%d grid=%d\n", what, row_len, count, f.waves, f.per,
                f.grid);
}

int main() {
  // (waves, per) detect_kernels.hip instantiates, ascending domains
  const int forms[][2] = {{1, 1}, {1, 2}, {1, 4}, {1, 8}, {4, 8}, {16, 8}, {16, 64}};
  const int counts[] = {1, 2, 3, 37, 511, 512, 513, 2047, 2048, 2049, 8191, 8192, 8193, 69632, 1 << 26, INT32_MAX};
  long n = 0;
  for (int row_len = 1; row_len <= kDetectMaxCols; ++row_len)
    for (int count : counts) {
      const DetectForm f = choose_detect(row_len, count);
      ++n;
      check(f.ok(), "a form for every width", row_len, count, f);
      if (!f.ok()) continue;
      check(row_len <= f.cols(), "the form's domain holds the row", row_len, count, f);
      int idx = -1;
      for (int k = 0; k < 7; ++k)
        if (forms[k][0] == f.waves && forms[k][1] == f.per) idx = k;
      check(idx >= 0, "a form the kernel file has", row_len, count, f);
      check(idx <= 0 || row_len > kDetectWord * forms[idx - 1][0] * forms[idx - 1][1], "the narrowest such form",
            row_len, count, f);
      check(f.waves >= 1 && f.waves <= 16 && 64 * f.waves <= 1024, "a workgroup of at most 1024 threads", row_len,
            count, f);
      check(row_len > 512 || f.waves == 1, "narrow rows: one wave per row", row_len, count, f);
      check(f.grid >= 1 && f.grid <= count && (int64_t)f.grid * f.waves <= 8192, "grid within the rows and one round",
            row_len, count, f);
      // the crossovers depend on row_len alone
      const DetectForm one = choose_detect(row_len, 1);
      check(one.waves == f.waves && one.per == f.per, "the form does not depend on count", row_len, count, f);
    }
  for (int row_len : {0, -1, kDetectMaxCols + 1, INT32_MIN, INT32_MAX})
    for (int count : {1, 37}) check(!choose_detect(row_len, count).ok(), "refused width", row_len, count, DetectForm());
  for (int count : {0, -1, INT32_MIN}) check(!choose_detect(512, count).ok(), "refused count", 512, count, DetectForm());
  if (g_bad) {
    std::printf("detect_form_sweep: %ld checks failed over %ld keys\n", g_bad, n);
    return 1;
  }
  std::printf("detect_form_sweep: ok (%ld keys)\n", n);
  return 0;
}
