// Prints the FC decimator's range-checked requests (pypanadapter_amd/csrc/fc_prefetch_plan.h,
// the functions fc_kernels.hip builds each request's buffer resource from) for
// tests/test_fc_tail_ranges.py:
//   lane EB T OFF                     the lane's byte offset into a request's resource
//   req Z DT L B MORE J BASE SIZE     request J of block B's window in a frame of L samples:
//                                     the resource's first byte (from the frame's) and its size
// for every format that takes them, every block B >= 1 with MORE = 1 (a block follows: the
// kernel requests it) and the window after the frame's last with MORE = 0.
// usage: fc_tail_ranges_dump Z L [L ...]         Plain g++, no HIP.
#include <cstdio>
#include <cstdlib>

#include "fc_prefetch_plan.h"

using namespace zfft::fc;

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  const int Z = std::atoi(argv[1]);
  const int S = pf_step(Z), KEEP = 16 - S, P = 512 * S / Z;
  const int dts[] = {kPfC64, kPfC32H, kPfF32R};
  const int ebs[] = {4, 8};
  for (int eb : ebs)
    for (int t = 0; t < 256; ++t) std::printf("lane %d %d %d\n", eb, t, pf_lane_off(t, eb));
  for (int a = 2; a < argc; ++a) {
    const long long L = std::atoll(argv[a]);
    const long long nd = (L + Z - 1) / Z;          // log2(Z) times ceil(n / 2)
    const int nb = (int)((nd + P - 1) / P);        // fc_decim_kernel's blocks per frame
    for (int DT : dts) {
      if (!pf_tail(Z, DT, 0)) return 3;
      const int eb = pf_elem_bytes(DT);
      for (int b = 1; b <= nb; ++b) {
        const bool more = b < nb;
        const long long s = pf_window_start(Z, b);
        const int left = pf_left_bytes(L, s, eb, more);
        for (int j = KEEP; j < 16; ++j)
          std::printf("req %d %d %lld %d %d %d %lld %d\n", Z, DT, L, b, (int)more, j,
                      s * eb + pf_req_base(j, eb), pf_req_bytes(left, j, eb));
      }
    }
  }
  return 0;
}
