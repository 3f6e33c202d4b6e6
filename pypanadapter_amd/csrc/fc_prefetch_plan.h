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

}  // namespace fc
}  // namespace zfft
