// fc_prefetch_plan.h -- where in a block the FC decimator (fc_kernels.hip) requests
// the next window's new pairs.  A thread holds 16 pairs of a window; the last KEEP = 16 - S of
// them are the next window's first KEEP and stay in registers, the other S are loaded while the
// block computes.  The plan says how many of those S are requested at each of five points of the
// block, in pair order: group g asks for the pairs KEEP + pf_first(g) .. + pf_count(g) - 1.
// Plain constexpr C++ (no HIP): tests/host/fc_prefetch_plan_dump.cpp prints the same tables the
// kernel is compiled from, tests/test_fc_prefetch_plan.py checks them.
#pragma once

// Build knobs (build(defines=...)), the defaults are what ships:
#ifndef FC_PARENT
#define FC_PARENT 0  // 1 = the block as before the spread prefetch: request schedule, hold, output stores
#endif
#ifndef FC_PF_SPREAD
#define FC_PF_SPREAD (!FC_PARENT)  // 0 = all of the next window requested at the block head
#endif
#ifndef FC_PF1
#define FC_PF1 10  // zoom 2, complex64: pairs of the next window requested at the block head
#endif
#ifndef FC_STEP
#define FC_STEP 13  // zoom 8's step (zfft_internal.h)
#endif
#ifndef FC_TAIL_CARRY
#define FC_TAIL_CARRY 1  // 0 = one resource per frame and a clamped window start: a frame's last window reloads
#endif
// Diagnostic overrides of the zoom-8 / zoom-4 plans, five counts: -DFC_PF_PLAN8=4,4,3,0,2

namespace zfft {
namespace fc {

// the points of a block, in program order
enum PfPoint {
  kPfHead = 0,    // the block head, after the window's values are taken
  kPfAfterA = 1,  // after pass A's LDS stores, before its barrier
  kPfAfterB = 2,  // after pass B's LDS stores, before its barrier
  kPfMidC = 3,    // between the two halves of pass C's rounds
  kPfAfterC = 4,  // after the barrier that ends pass C
  kPfPoints = 5
};
// input formats as zfft_internal.h's InDtype numbers them (fc_kernels.hip asserts the match)
constexpr int kPfC64 = 0, kPfC32H = 1, kPfCU8 = 2, kPfF32R = 3;

// a block advances 512 S samples: S new pairs per thread and window
constexpr int pf_step(int Z) { return Z == 8 ? FC_STEP : Z == 4 ? 14 : 15; }

struct PfPlan {
  int n[kPfPoints];
};

// Which instantiations request in pieces (and with that hold more of the filter table and store
// through a buffer resource, fc_kernels.hip).  Not zoom 2, which keeps its split for register
// room, and not cu8: the byte unpacking of a pair is placed right behind its load, so every
// pinned group is waited for where it is issued.
constexpr bool pf_spread(int Z, int DT) { return FC_PF_SPREAD && Z != 2 && DT != kPfCU8; }

// An in-order counter completes the requests, so a wait for a filter-table pair in pass C also
// takes every group issued before it.
constexpr PfPlan pf_plan(int Z, int DT, int FLIP) {
  (void)FLIP;
  const int S = pf_step(Z);
  if (Z == 2) return DT == kPfC64 ? PfPlan{{FC_PF1, 0, 0, 0, S - FC_PF1}} : PfPlan{{S, 0, 0, 0, 0}};
  if (!pf_spread(Z, DT)) return PfPlan{{S, 0, 0, 0, 0}};
#ifdef FC_PF_PLAN8
  if (Z == 8) return PfPlan{{FC_PF_PLAN8}};
#endif
#ifdef FC_PF_PLAN4
  if (Z == 4) return PfPlan{{FC_PF_PLAN4}};
#endif
  // Four at the head, four after pass A, the rest behind pass C: pass C keeps its registers, and
  // zoom 4 complex64, which still reads 3 of its 16 table pairs per block right after pass B's
  // barrier, has no group shortly before them.  Five or six requests land in the inverse's time,
  // nine do not (the measured plans: DESIGN §3.9).
  return PfPlan{{4, 4, 0, 0, S - 8}};
}

constexpr int pf_count(int Z, int DT, int FLIP, int g) { return pf_plan(Z, DT, FLIP).n[g]; }
// index (among the S new pairs) of group g's first
constexpr int pf_first(int Z, int DT, int FLIP, int g) {
  int s = 0;
  for (int i = 0; i < g; ++i) s += pf_plan(Z, DT, FLIP).n[i];
  return s;
}
constexpr int pf_total(int Z, int DT, int FLIP) { return pf_first(Z, DT, FLIP, kPfPoints); }
constexpr bool pf_valid(int Z, int DT, int FLIP) {
  for (int g = 0; g < kPfPoints; ++g)
    if (pf_count(Z, DT, FLIP, g) < 0) return false;
  return pf_total(Z, DT, FLIP) == pf_step(Z);
}

// Range-checked requests (FC_TAIL_CARRY).  Request j of a window that starts at sample s >= 0 of
// a frame of L samples is the 512 samples from s + 512 j on, a pair (2t, 2t + 1) of them per lane
// t.  It goes through a buffer resource of its own: the base is the request's first byte, the
// size the frame's bytes left from there, at most the request's, and the lane's offset is all
// the address there is, so the range check returns exactly the frame's samples and 0 past its
// end, dword by dword (a pair that straddles the end gives one sample and one 0; every element
// here is whole dwords), whatever the hardware does with a scalar offset.  With that a window
// that overhangs the frame's end is requested like any other, and only a run's first window,
// which may start before the frame, loads sample by sample.
// Which instantiations: those that request in pieces, without FLIP (mirrored offsets run down
// and past the frame's first byte).  Not cu8 (raw 0 is not the value 0, and half a dword).
constexpr bool pf_tail(int Z, int DT, int FLIP) { return FC_TAIL_CARRY && pf_spread(Z, DT) && !FLIP; }
constexpr int pf_elem_bytes(int DT) { return DT == kPfC64 ? 8 : DT == kPfCU8 ? 2 : 4; }
// first sample of block b's window: the blocks advance 512 S samples, the window reaches
// K = (8192 - 512 S) / 2 before the block's first (fc_kernels.hip asserts its own against this)
constexpr long long pf_window_start(int Z, int b) { return 512LL * pf_step(Z) * b - (8192 - 512 * pf_step(Z)) / 2; }
// bytes of the frame from the window start on (0 <= s <= L, and a frame FC takes has < 2^31
// bytes: 32-bit scalar arithmetic throughout); 0 when no block follows (more = 0), so that a
// run's last block requests nothing of a window nobody takes
constexpr int pf_left_bytes(long long L, long long s, int eb, bool more) { return more ? (int)((L - s) * eb) : 0; }
// the request's first byte from the window's first
constexpr int pf_req_base(int j, int eb) { return 512 * eb * j; }
// the size of its resource
constexpr int pf_req_bytes(int left, int j, int eb) {
  const int r = left - pf_req_base(j, eb);
  return r < 0 ? 0 : r > 512 * eb ? 512 * eb : r;
}
// the lane's offset into it
constexpr int pf_lane_off(int t, int eb) { return 2 * t * eb; }

}  // namespace fc
}  // namespace zfft
