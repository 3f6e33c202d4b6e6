// zfft_dif_addr.h -- LDS slot arithmetic and the window-hold rule of the in-place DIF Welch kernel
// (welch_dif_kernel, zfft_kernels.hip).  Plain constexpr C++ (no HIP):
// tests/host/dif_addr_check.cpp walks the same functions the kernel is compiled from,
// tests/test_welch_dif_addr.py runs it.
#pragma once

// Build knobs (build(defines=...)), the defaults are what ships; 0 restores the code of before:
#ifndef ZFFT_DIF_CADDR
#define ZFFT_DIF_CADDR 1  // stage stores/loads at one base per segment plus constant slot offsets
#endif                    // (0: dif_slot() of every index, rebuilt per value)
#ifndef ZFFT_DIF_WHOLD
#define ZFFT_DIF_WHOLD 1  // window values held in registers across the segments (0: none held,
#endif                    // all 16 re-read every segment)
#ifndef ZFFT_DIF_PFPIN
#define ZFFT_DIF_PFPIN 1  // the next segment's prefetch pinned at the segment head by a scheduling
#endif                    // barrier behind it.  No time of its own at cfg2, cfg1 or cfg3 (with the
                          // window loads gone the compiler requests at the head by itself there,
                          // profiles/welch_regs); kept for the registers: with 0 the two N = 1024
                          // pruned non-overlap sum forms spill 2 VGPRs (tests/test_welch_build.py)

namespace zfft {
namespace dif {

// LDS slot of element i: one pad slot per 16 elements (conflict-free strides 1, 16, 17)
constexpr int slot(int i) { return i + (i >> 4); }

// A thread's accesses of one stage are base + stride * k, k < 16, stride a power of two.  When
// (base & 15) + ((stride * k) & 15) < 16 for every k the pad of the sum is the sum of the pads,
//   slot(base + stride k) = slot(base) + slot(stride k),
// so one address per segment and sixteen constants do.  That holds for
//   stage 1:       base = t < T, stride T (a multiple of 16): slot(T k) = (T + T/16) k
//   middle stages: base = (t / S) 16 S + (t mod S), stride S = N / 16^st: for S < 16 the low bits
//                  of base are t mod S < S and stride k mod 16 is a multiple of S, at most 16 - S
//   last stage:    base = 16 t, stride 1.
constexpr int slot_off(int stride, int k) { return slot(stride * k); }
constexpr int mid_base(int t, int S) { return (t / S) * (16 * S) + (t & (S - 1)); }

// The DS instructions' offset field is 16 bits of bytes: a slot is 8 bytes
constexpr int kMaxImmSlots = 65535 / 8;
// first k of a stage with this stride whose offset needs a second base (16: none)
constexpr int second_base_from(int stride) {
  for (int k = 0; k < 16; ++k)
    if (slot_off(stride, k) > kMaxImmSlots) return k;
  return 16;
}

// Window values (of a thread's 16) held in registers for the whole kernel, by instantiation: as
// many as the register bound of its launch bound (waves per SIMD: 128 VGPRs at 4, 168 at 3, 256
// at 2) leaves without a spill and without lowering the occupancy; the others are re-read every
// segment.  tests/test_welch_build.py checks the bound on every instantiation.
constexpr int win_hold(int N, bool prune, bool half, bool seg, bool lines) {
  (void)lines;
  if (!ZFFT_DIF_WHOLD) return 0;
  // N = 4096 at 3 waves/SIMD (168): the pruned 50 %-overlap form (the batch headline) compiles
  // to 142 VGPRs without the window and takes all 16; the other forms sit at 156-168 already
  if (N == 4096) return prune && half ? 16 : 0;
  // N = 8192: the 50 %-overlap forms fit 168 VGPRs (3 waves/SIMD) only without the window, the
  // others are at 2 waves/SIMD either way and have the room
  if (N == 8192) return half ? 0 : 16;
  // N <= 2048, full last stage, 3 waves/SIMD; the pruned form (4 waves/SIMD, 128) holds none
  if (N <= 2048 && !prune) return seg ? 16 : 8;
  return 0;  // N = 16384: a 1024-thread workgroup, 128 VGPRs
}

}  // namespace dif
}  // namespace zfft
