// fc_kernels.hip -- "FC", the fast-convolution form of the zoom-8 decimator on gfx950 (host
// tables: fc_build_table in pc_tables.cpp; design model: tools/fc_model.py), of
// zoom 4 (four residues of 2048 points) and of zoom 2 (path 7: two residues of 4096 points, the
// one-stage model truncated at |k| <= 256, 3840 outputs per window).  Zoom 8:
//
// The interior of three scipy.signal.decimate(x, 2) (pypanadapter_spectrum.py:2096-2098) is the
// zero-phase LTI filter G = prod_k |H(z^(2^k))|^2 on the zero-extended frame followed by [::8]
// (DESIGN §3.5).  Its input-rate impulse response g falls below 1.0e-6 of sum |g| beyond
// |k| = kFcK = 768 (1.4e-8 beyond 1024; tools/fc_model.py); truncated there it is applied by
// overlap-save FFT convolution, one 8192-sample window per block:
//   block b: window w[n] = x[6656 b - 768 + n], n < 8192 (zero outside the frame)
//   residues a_r[m] = w[8m + r]: eight 1024-point DFTs A_r (radix 16, 16, 4; decimation in
//            frequency, in lock step: the residues share every twiddle)
//   Yf[k] = sum_r A_r[k] C[k][r],  C[k][r] = W_8192^(rk) sum_q G[k + 1024 q] W_8^(rq) / 8192
//            -- the [::8] is an alias sum in frequency, here fused with the filter
//   y[j] = IDFT_1024(Yf)[j] (five radix-4 stages), outputs m = 832 b + j - 96, j in [96, 928)
// The LO mix moves into the filter: (x lo) * g at 8m equals lo[8m] (x * g') with
// g'[k] = g[k] e^(2 pi i f_lo k / fs) (lo[n] = sqrt 2 e^(-2 pi i f_lo n / fs) is an exact
// exponential), so C holds the modulated filter's spectrum (one table per LO row) and each output
// takes lo[8m] once, as the composite lo[6656 b] lo[8 (j - 96)] / sqrt 2.
// Frame ends: the walk's maps (pc_edge_batch_kernel behind this kernel on its stream: exact
// minus the zero-extended model), which g's truncation changes by < 2e-8.
//
// Work per input sample: ~30 VALU lane-instructions (the walk: 74); LDS: two
// exchanges of the 8192-point window plus three small ones of the 1024-point inverse per block
// (inverse stages 2..4 exchange between a wave's lanes in registers).
#include <algorithm>
#include <type_traits>

#include "fc_prefetch_plan.h"
#include "zfft_device.h"
#include "zfft_fft.h"
#include "zfft_pairs.h"

// Diagnostic builds only (ZFFT_DIAG=1, never set by build.py), timing knockouts with wrong
// results by design: FC_KO 1 the input loads (window values from registers), 2 the filter-table
// loads, 4 the output stores (profiles/r06fc/r06fc4: 2.84 ms -> 1.85 / 2.61 / 2.54, all three
// 1.56 at K = 1024).  Measured and removed: the filter table requested before the prefetch
// (2.98 ms, spills) and the prefetch requested after the table (2.80, r06fc5; again with the
// block head's drain gone: 3.17 against 3.00 ms per step, r07fc) and the table requested before
// the barrier that ends pass B (2.90 against 2.88, r07fc).
#ifndef ZFFT_DIAG
#define ZFFT_DIAG 0
#endif
#if !ZFFT_DIAG && defined(FC_KO)
#error "FC_KO is a diagnostic knob: build with -DZFFT_DIAG"
#endif
#ifndef FC_KO
#define FC_KO 0
#endif
// A/B knobs (build(defines=...)), the defaults are what ships:
#ifndef FC_INV_LDS
#define FC_INV_LDS 0  // 1 = inverse stages 2..4 exchange through LDS instead of between lanes
#endif
#ifndef FC_HEAD_DRAIN
#define FC_HEAD_DRAIN 0  // 1 = the block head as before: no wait closing the edge path, plain pointers
#endif
#ifndef FC_CTAB_ORDER
#define FC_CTAB_ORDER 1  // 0 = pass C's table pairs held and requested in storage order
#endif
#if FC_HEAD_DRAIN
#define FC_RESTRICT
#else
#define FC_RESTRICT __restrict__
#endif
// FC_PARENT, FC_PF_SPREAD, FC_PF1: fc_prefetch_plan.h (the request schedule of the next window)
#ifndef FC_OUT_BUF
#define FC_OUT_BUF (!FC_PARENT)  // 0 = the outputs stored under a lane condition, through plain pointers
#endif
#ifndef FC_HOLD
#define FC_HOLD (-1)  // diagnostic override of fc_hold for every non-cu8 instantiation
#endif


namespace zfft {
namespace fc {

typedef v2f __attribute__((address_space(3))) *LP;
typedef v4f __attribute__((address_space(3))) *LP4;

// Block geometry per zoom (zfft_internal.h): Z residues of an M = 8192 / Z point DFT; a block
// advances 512 S samples and makes P = 512 S / Z outputs; K = (8192 - 512 S) / 2.
template <int Z> struct Geo;
template <> struct Geo<8> { static constexpr int S = kFcStep, K = kFcK, P = kFcP; };
template <> struct Geo<4> { static constexpr int S = kFc4Step, K = kFc4K, P = kFc4P; };
template <> struct Geo<2> { static constexpr int S = kFc2Step, K = kFc2K, P = kFc2P; };
constexpr int kN = kFcN;
// LDS: the window as [pos][residue] with 2 pad slots per 32 (conflict-free b128 reads in all
// three forward passes, tools/fc_model.py layout check); the inverse M points, 1 pad per 16 --
// its own array at zoom 8 (1024 points), inside the window's at zoom 4 and 2 (2048 / 4096: two
// arrays would not fit two workgroups per CU)
constexpr int kBigSlots = kN + 2 * (kN / 32);
constexpr int kSmallSlots8 = 1024 + 1024 / 16;
// Zoom 2 pads once more per 256: stage 5's lanes read 256 b0 apart for 16 values of b0 (R1), which
// 1 per 16 alone leaves on two bank groups (8-way; 4-way at zoom 4's 8 values, 2-way at zoom 8)
template <int Z>
__device__ __forceinline__ int ps(int i) { return i + (i >> 4) + (Z == 2 ? i >> 8 : 0); }

// acc + a b (complex) in two VOP3P instructions (cmul2 with the accumulator as the addend)
__device__ __forceinline__ v2f cmac2(v2f acc, v2f a, v2f b) {
  v2f t, r;
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1]" : "=v"(t) : "v"(a), "v"(b), "v"(acc));
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]"
      : "=v"(r) : "v"(a), "v"(b), "v"(t));
  return r;
}
__device__ __forceinline__ v2f conj(v2f a) { return v2f{a.x, -a.y}; }
// sum_a v_a W_R^(-ab): the forward radix R with outputs b and R - b exchanged
template <int R>
__device__ __forceinline__ void idft(v2f *v) {
  dft<R>(v);
#pragma unroll
  for (int b = 1; b < R / 2; ++b) {
    const v2f s = v[b];
    v[b] = v[R - b];
    v[R - b] = s;
  }
}
// v[b] *= w^b, b = 1 .. R-1 (R = 4, 8, 16)
template <int R>
__device__ __forceinline__ void pow_tw(v2f *v, v2f w);
template <>
__device__ __forceinline__ void pow_tw<4>(v2f *v, v2f w) {
  const v2f w2 = cmul2(w, w);
  v[1] = cmul2(v[1], w);
  v[2] = cmul2(v[2], w2);
  v[3] = cmul2(v[3], cmul2(w2, w));
}
template <>
__device__ __forceinline__ void pow_tw<8>(v2f *v, v2f w) {  // each power from at most 3 products
  const v2f w2 = cmul2(w, w), w4 = cmul2(w2, w2), w3 = cmul2(w2, w);
  v[1] = cmul2(v[1], w);
  v[2] = cmul2(v[2], w2);
  v[3] = cmul2(v[3], w3);
  v[4] = cmul2(v[4], w4);
  v[5] = cmul2(v[5], cmul2(w4, w));
  v[6] = cmul2(v[6], cmul2(w4, w2));
  v[7] = cmul2(v[7], cmul2(w4, w3));
}

template <>
__device__ __forceinline__ void pow_tw<16>(v2f *v, v2f w) {  // each power from at most 4 products
  const v2f w2 = cmul2(w, w), w4 = cmul2(w2, w2), w8 = cmul2(w4, w4), w3 = cmul2(w2, w);
  const v2f w5 = cmul2(w4, w), w6 = cmul2(w4, w2), w7 = cmul2(w4, w3);
  v[1] = cmul2(v[1], w);
  v[2] = cmul2(v[2], w2);
  v[3] = cmul2(v[3], w3);
  v[4] = cmul2(v[4], w4);
  v[5] = cmul2(v[5], w5);
  v[6] = cmul2(v[6], w6);
  v[7] = cmul2(v[7], w7);
  v[8] = cmul2(v[8], w8);
  v[9] = cmul2(v[9], cmul2(w8, w));
  v[10] = cmul2(v[10], cmul2(w8, w2));
  v[11] = cmul2(v[11], cmul2(w8, w3));
  v[12] = cmul2(v[12], cmul2(w8, w4));
  v[13] = cmul2(v[13], cmul2(w8, w5));
  v[14] = cmul2(v[14], cmul2(w8, w6));
  v[15] = cmul2(v[15], cmul2(w8, w7));
}

// Loads through buffer resources: one lane offset VGPR and constant SGPR offsets per load (64-bit
// addresses per load, hoisted out of the block loop, spilled 60-100 VGPRs), and a load past the
// resource's end returns 0 (the window's samples outside the frame).
constexpr int kBufFlags = 0x00020000;
template <int DT>
constexpr int ebytes() { return DT == kInC64 ? 8 : DT == kInCU8 ? 2 : 4; }
template <int DT>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t frame_rsrc(const InDesc &in, int64_t f) {
  constexpr int eb = ebytes<DT>();
  return __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)in.p + f * in.stride * eb), (short)0,
                                           (int)(in.len * eb), kBufFlags);
}
// sample n of the frame, 0 outside it (the load returns raw 0 there, which is -1 - 1i for cu8:
// the value is selected after the conversion)
template <int DT, int FLIP>
__device__ __forceinline__ v2f load_sample(__amdgpu_buffer_rsrc_t rs, int64_t L, int64_t n) {
  constexpr int eb = ebytes<DT>();
  const int64_t k = FLIP ? L - 1 - n : n;
  const bool in = n >= 0 && n < L;
  const uint32_t vo = in ? (uint32_t)(k * eb) : 0x80000000u;
  if constexpr (DT == kInC64) {
    return __builtin_bit_cast(v2f, __builtin_amdgcn_raw_buffer_load_b64(rs, vo, 0, 0));
  } else if constexpr (DT == kInC32H) {
    const h2 h = __builtin_bit_cast(h2, __builtin_amdgcn_raw_buffer_load_b32(rs, vo, 0, 0));
    return v2f{(float)h.x, (float)h.y};
  } else if constexpr (DT == kInF32R) {
    return v2f{__builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, vo, 0, 0)), 0.f};
  } else {
    const u8x2 u = __builtin_bit_cast(u8x2, __builtin_amdgcn_raw_buffer_load_b16(rs, vo, 0, 0));
    const v2f v{((float)u.x - 127.5f) * (1.f / 127.5f), ((float)u.y - 127.5f) * (1.f / 127.5f)};
    return in ? v : splat(0.f);
  }
}
// load_sample in 32-bit sample numbers (no FLIP, no cu8; a frame is < 2^31 bytes): one unsigned
// compare per sample and no 64-bit lane value kept across the block loop for a run's first block
template <int DT>
__device__ __forceinline__ v2f load_sample32(__amdgpu_buffer_rsrc_t rs, int L, int n) {
  static_assert(DT != kInCU8, "raw 0 is not cu8's 0");
  const uint32_t vo = (uint32_t)n < (uint32_t)L ? (uint32_t)n * ebytes<DT>() : 0x80000000u;
  if constexpr (DT == kInC64) {
    return __builtin_bit_cast(v2f, __builtin_amdgcn_raw_buffer_load_b64(rs, vo, 0, 0));
  } else if constexpr (DT == kInC32H) {
    const h2 h = __builtin_bit_cast(h2, __builtin_amdgcn_raw_buffer_load_b32(rs, vo, 0, 0));
    return v2f{(float)h.x, (float)h.y};
  } else {
    return v2f{__builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, vo, 0, 0)), 0.f};
  }
}
// the raw pair (n, n + 1), n = s + 2t + 512 j, of a window inside the frame: voffset from
// pair_vo (per block), soffset the constant 512 eb j (mirrored for FLIP)
template <int DT, int FLIP>
__device__ __forceinline__ uint32_t pair_vo(int64_t L, int64_t s, int t) {
  constexpr int eb = ebytes<DT>();
  return (uint32_t)((FLIP ? L - 2 - s - 7680 - 2 * t : s + 2 * t) * eb);
}
template <int DT>
__device__ __forceinline__ typename RawP<DT>::T load_pair_raw(__amdgpu_buffer_rsrc_t rs, uint32_t vo, int so) {
  typedef typename RawP<DT>::T T;
  constexpr int aux = 2;  // non-temporal: the window is streamed once (-1 % per step, r06fc6)
  if constexpr (DT == kInC64) return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b128(rs, vo, so, aux));
  else if constexpr (DT == kInCU8) return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b32(rs, vo, so, aux));
  else return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b64(rs, vo, so, aux));
}
template <int DT, int FLIP>
__device__ __forceinline__ typename RawP<DT>::T load_pair_b(__amdgpu_buffer_rsrc_t rs, uint32_t vo, int j) {
  constexpr int eb = ebytes<DT>();
  return load_pair_raw<DT>(rs, vo, 512 * eb * (FLIP ? 15 - j : j));
}
// FC_TAIL_CARRY (fc_prefetch_plan.h; no FLIP, no cu8): request j of the window whose first byte
// is w and from which the frame has `left` bytes, through a resource of its own -- its first
// byte, its bytes inside the frame -- with the lane's offset pf_lane_off alone, so the pair
// comes back as load_sample gives its two samples: 0 where the frame has ended.  All scalar.
template <int DT>
__device__ __forceinline__ typename RawP<DT>::T load_pair_r(const char *w, int left, uint32_t vo, int j) {
  constexpr int eb = ebytes<DT>();
  static_assert(DT != kInCU8 && eb % 4 == 0, "whole dwords per sample: the range check is per dword");
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      (void *)(w + pf_req_base(j, eb)), (short)0, pf_req_bytes(left, j, eb), kBufFlags);
  return load_pair_raw<DT>(rs, vo, 0);
}
// Between two inverse stages whose elements stay inside one wave, the exchange is a 4 x 4
// transpose of a lane's register index a against two bits of its lane number, one bit at a time
// and one dword at a time (tests/test_fc_lane_exchange.py models exactly this sequence).
// Bits 5:4 (stage 2 -> 3): v_permlane32_swap exchanges the upper 32 lanes of its first operand
// with the lower 32 of its second, v_permlane16_swap the odd 16-lane rows of the first with the
// even rows of the second.  (fbits takes the float by value: __builtin_bit_cast applied to a
// vector element through a reference read element 0 for .y as well.)
__device__ __forceinline__ unsigned fbits(float f) { return __builtin_bit_cast(unsigned, f); }
__device__ __forceinline__ float bitsf(unsigned u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ void swap32(v2f &a, v2f &b) {
  const auto x = __builtin_amdgcn_permlane32_swap(fbits(a.x), fbits(b.x), false, false);
  const auto y = __builtin_amdgcn_permlane32_swap(fbits(a.y), fbits(b.y), false, false);
  a = v2f{bitsf(x[0]), bitsf(y[0])};
  b = v2f{bitsf(x[1]), bitsf(y[1])};
}
__device__ __forceinline__ void swap16(v2f &a, v2f &b) {
  const auto x = __builtin_amdgcn_permlane16_swap(fbits(a.x), fbits(b.x), false, false);
  const auto y = __builtin_amdgcn_permlane16_swap(fbits(a.y), fbits(b.y), false, false);
  a = v2f{bitsf(x[0]), bitsf(y[0])};
  b = v2f{bitsf(x[1]), bitsf(y[1])};
}
// Bits 3:2 (stage 3 -> 4), inside a 16-lane row: the lanes with lane bit SH set take b from SH
// lanes below into a (DPP row_shr, bank mask = those lanes' banks of 4), the others a from SH
// lanes above into b (row_shl); a masked-off lane keeps what it had.
template <int SH>
__device__ __forceinline__ void swap_row(v2f &a, v2f &b) {
  constexpr int hi = SH == 8 ? 0xc : 0xa, lo = 0xf ^ hi;
  const unsigned ax = fbits(a.x), ay = fbits(a.y), bx = fbits(b.x), by = fbits(b.y);
  a = v2f{bitsf(__builtin_amdgcn_update_dpp(ax, bx, 0x110 + SH, 0xf, hi, false)),
          bitsf(__builtin_amdgcn_update_dpp(ay, by, 0x110 + SH, 0xf, hi, false))};
  b = v2f{bitsf(__builtin_amdgcn_update_dpp(bx, ax, 0x100 + SH, 0xf, lo, false)),
          bitsf(__builtin_amdgcn_update_dpp(by, ay, 0x100 + SH, 0xf, lo, false))};
}
// lane l, register a: element l + 64 a -> (l & 15) + 16 a + 64 (l >> 4)
__device__ __forceinline__ void xchg_54(v2f *v) {
  swap32(v[0], v[2]);
  swap32(v[1], v[3]);
  swap16(v[0], v[1]);
  swap16(v[2], v[3]);
}
// -> (l & 3) + 4 a + 16 ((l >> 2) & 3) + 64 (l >> 4)
__device__ __forceinline__ void xchg_32(v2f *v) {
  swap_row<8>(v[0], v[2]);
  swap_row<8>(v[1], v[3]);
  swap_row<4>(v[0], v[1]);
  swap_row<4>(v[2], v[3]);
}
#if FC_INV_LDS
// the LDS form of the same exchanges: a wave's LDS operations complete in issue order, so
// ordering the compiler's view (wavefront-scope fences around a wave barrier) is all it takes
__device__ __forceinline__ void stage_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
#endif

// How many of a thread's 16 C pairs stay in registers for the whole kernel instead of being
// re-read from L2 every block: as many as each instantiation holds without spilling at 2 WG/CU
// (cu8 has no room; against none, complex64 8 at zoom 8: fc_decim 2.62 -> 2.55 ms at cfg2,
// r06fc10; 6 at zoom 4 and 14 for complex32 beat 4 and 12 by 1.1 / 0.6 % per step, r06fc13).
// Zoom 2 holds none: pass C is one round of 32 values against all 16 pairs, and complex64
// spills 13-19 registers even so unless part of the prefetch moves behind it (FC_PF1).
// With the next window requested in pieces (fc_prefetch_plan.h) its registers fill as the block
// goes instead of all being live from the block head, and the room goes to the table: all 16
// pairs, so pass C issues no load at all and nothing in the block loop waits for the table
// (with the spread: cfg2 -3.9 % per step, cfg1 -5.1 %, complex32 -3.3 %, profiles/r09fcpf); 13
// for complex64 at zoom 4 (14 spills 2 registers).  The values of before where the requests are not spread (cu8, FC_PARENT).
constexpr int fc_hold(int Z, int DT) {
  if (Z == 2) return 0;
  if (!pf_spread(Z, DT)) return DT == kInCU8 ? 0 : DT == kInC64 ? (Z == 8 ? 8 : 6) : 14;
  return DT == kInC64 && Z == 4 ? 13 : 16;
}

// One workgroup walks blocks [bpc * blockIdx.x, +bpc) of frame blockIdx.y.  tab: W_M^k (k < M),
// then per LO row (row_stride apart) C as v4f pairs [(Z / 2) k3 + r / 2][t] (r, r + 1) for thread t
// of pass C.  Needs frames of >= kFcN samples and < 2^31 bytes (launch_fc_decim); at zoom 2 an
// LO row of > 4096 entries (the composite below; every caller's frames have >= 16384 samples).
template <int Z, int DT, int FLIP>
__global__ void __launch_bounds__(256, 2) fc_decim_kernel(InDesc in, const v2f *FC_RESTRICT lo,
                                                         const v2f *FC_RESTRICT tab, int64_t row_stride,
                                                         v2f *FC_RESTRICT out, int64_t nd, int bpc) {
  constexpr int M = kN / Z;             // per-residue transform: 1024 (zoom 8), 2048 (4), 4096 (2)
  constexpr int R1 = M / 256;           // radix of the last forward / first inverse stage
  constexpr int S = Geo<Z>::S, K = Geo<Z>::K, P = Geo<Z>::P;
  constexpr int KEEP = 16 - S;          // a thread's pairs carried into the next window
  constexpr int J0 = K / Z;             // first valid inverse output
  constexpr int NB = M / 1024;          // inverse butterflies per thread in stages 2..5
  constexpr bool ALIAS = Z != 8;        // the inverse array inside the window's
  static_assert(K == (kN - 512 * S) / 2 && P * Z == 512 * S && K % Z == 0 && KEEP >= 1, "FC block geometry");
  static_assert(J0 + P <= M && J0 < 256 * NB, "FC outputs");
  static_assert(!ALIAS || M + M / 16 + M / 256 <= kBigSlots, "the inverse array inside the window's");
  __shared__ v4f big4[kBigSlots / 2];
  __shared__ v2f small_[ALIAS ? 2 : kSmallSlots8];
  const LP bl = (LP)big4;
  const LP sl = ALIAS ? bl : (LP)small_;
  const int t = threadIdx.x;
  const int64_t f = blockIdx.y, L = in.len;
  const int nb = (int)((nd + P - 1) / P);
  const int b0 = (int)blockIdx.x * bpc, b1 = min(nb, b0 + bpc);
  if (b0 >= b1) return;
  const v2f *lor = lo_row(lo, in, f);
  const int row = in.lo_n <= 1 ? 0 : (int)((((int64_t)in.lo_first + f) / in.lo_per) % in.lo_n);
  const v2f *tw = tab;
  const __amdgpu_buffer_rsrc_t crs =
      __builtin_amdgcn_make_buffer_rsrc((void *)(tab + M + row * row_stride), (short)0, kFcRow * 8, kBufFlags);
  const __amdgpu_buffer_rsrc_t xrs = frame_rsrc<DT>(in, f);
  // pass A: residues of thread t's pairs 2t + 512 i are (2t mod Z, +1), at m = j0 + (M / 16) i;
  // pass B: k1 = t >> 4, j1 = the digit below i2 of the (M / 16)-point remainder
  constexpr int ZS = Z == 8 ? 2 : Z == 4 ? 1 : 0;  // log2(Z / 2): a thread's pair 2t is position t >> ZS
  const int j0 = t >> ZS, j1 = (t >> ZS) & (15 >> ZS);
  v2f bA[4], bB[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    bA[s] = tw[(j0 << s) & (M - 1)];
    bB[s] = tw[((16 * j1) << s) & (M - 1)];
  }
  // pass C: k1 = t >> 4, k2 = t & 15 -> kp = k1 + 16 k2
  const int kp = (t >> 4) + 16 * (t & 15);
  // HOLD of its 16 C pairs held for the whole kernel, the rest read per block.  Pass C takes
  // pair (Z / 2) k + rp in its round rp: cix(j) is the j-th pair in that order, and the pairs are
  // held and requested in it, so the first rounds need no load and every later wait leaves
  // the requests of the rounds after it in flight.
  constexpr int HOLD = FC_HOLD >= 0 ? (DT == kInCU8 ? 0 : FC_HOLD) : fc_hold(Z, DT);
  auto cix = [](int j) { return FC_CTAB_ORDER ? (Z / 2) * (j % R1) + j / R1 : j; };
  v4f ch[HOLD > 0 ? HOLD : 1];
#pragma unroll
  for (int j = 0; j < HOLD; ++j)
    ch[j] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(crs, (uint32_t)(16 * t), 4096 * cix(j), 0));
  // inverse twiddle bases, conjugated: stage 1 W_M^kp, 2 W_256^(t & 63), 3 W_64^(t & 15),
  // 4 W_16^(t & 3) (the digits below each stage's)
  const v2f ib0 = conj(tw[kp]), ib1 = conj(tw[(M / 256) * (t & 63)]), ib2 = conj(tw[(M / 64) * (t & 15)]),
            ib3 = conj(tw[(M / 16) * (t & 3)]);
  // outputs: butterfly u = t + 256 h of stage 5 gives j = u + (M / 4) b4, valid for j in
  // [J0, J0 + P), at output jm = j - J0 of the block; their lo[Z jm] (0 where invalid / past
  // the frame)
  // Zoom 2 has no room for its 16 values: lo is an exact exponential of modulus sqrt 2, so
  // lo[Z jm] = lo[Z (t + 256 h + M / 4 - J0)] lo[Z (M / 4) (q - 1)] / sqrt 2 -- four per thread
  // (lt) and four uniform ones (lq; q = 0: the conjugate of q = 2's; divided by the table's
  // modulus lo[0] = sqrt 2, or 1 for a tail's unit table)
  constexpr bool LJ = Z != 2;
  v2f lj[LJ ? NB : 1][4], lt[LJ ? 1 : NB], lq[4];
  if constexpr (LJ) {
#pragma unroll
    for (int h = 0; h < NB; ++h)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int jm = t + 256 * h + (M / 4) * q - J0;
        lj[h][q] = jm >= 0 && jm < P && jm < nd ? lor[Z * jm] : splat(0.f);
      }
  } else {
#pragma unroll
    for (int h = 0; h < NB; ++h) lt[h] = lor[Z * (t + 256 * h + M / 4 - J0)];
#pragma unroll
    for (int q = 1; q < 4; ++q) lq[q] = lor[Z * (M / 4) * (q - 1)] * (1.f / lor[0].x);
    lq[0] = conj(lq[2]);
  }
  // LDS bases (v2f slots; the pads folded into the constant strides)
  const int aA = 2 * t + 2 * (t >> 4);                 // pb(512 k + 2t) = aA + 544 k
  const int aB = 2 * (t & 15) + 544 * (t >> 4);        // pb(base + 32 i) = aB + 34 i
  const int aC = 544 * (t >> 4) + 34 * (t & 15);       // pair p of pass C: aC + 2 p
  constexpr int Q1 = 272 + (Z == 2), H1 = 1088 + 4 * (Z == 2);  // ps(256), ps(1024)
  const int a1 = ps<Z>(kp);                            // ps(kp + 256 q) = a1 + Q1 q
  // stages 2..4 (butterfly t + 256 h at + H1 h), stage 5
  const int a2 = ps<Z>((t & 63) + 256 * (t >> 6));                                      // + 68 a
#if FC_INV_LDS
  const int a3 = ps<Z>((t & 15) + 64 * ((t >> 4) & 3) + 256 * (t >> 6));               // + 17 a
#endif
  const int a4 = ps<Z>((t & 3) + 16 * ((t >> 2) & 3) + 64 * ((t >> 4) & 3) + 256 * (t >> 6));  // + 4 a
  auto a5 = [&](int h) {  // u = b0 + R1 (b1 + 4 b2 + 16 b3) reads (a0 + 4 b3 + 16 b2 + 64 b1 + 256 b0)
    const int u = t + 256 * h, r = u / R1;
    return ps<Z>(4 * ((r >> 4) & 3) + 16 * ((r >> 2) & 3) + 64 * (r & 3) + 256 * (u % R1));
  };

  auto wstart = [&](int b) -> int64_t { return (int64_t)(512 * S) * b - K; };
  [[maybe_unused]] auto inside = [&](int b) { const int64_t s = wstart(b); return s >= 0 && s + kN <= L; };
  typename RawP<DT>::T pf[S];  // the next window's pairs KEEP .. 15
  v2f ka[KEEP], kb[KEEP];      // this window's pairs S .. 15 = the next window's 0 .. KEEP-1
  // TAIL: every request of the next window through a resource of its own, range-checked
  // against the frame's end (fc_prefetch_plan.h), and not through the frame's at a window start
  // clamped into the frame.  So every block after a run's first is carried, the frame's last,
  // overhanging window too: before, that block threw the 13 (14) requests away, reloaded the
  // whole window sample by sample and waited for it in the open -- once per frame, 2.2 % of
  // the kernel's bytes at cfg2.  The lane's offset is loop-invariant, the rest scalar (6
  // instructions a request).  FLIP (mirrored offsets, which run past the frame's first byte),
  // cu8 (its raw 0 is not the value 0) and zoom 2 keep the clamped start and compile to the
  // instructions of before, as does every instantiation with FC_TAIL_CARRY=0 (compared
  // function by function on hipcc -S).
  constexpr bool TAIL = pf_tail(Z, DT, FLIP);
  static_assert(!TAIL || (Z != 2 && DT != kInCU8 && !FLIP && pf_elem_bytes(DT) == ebytes<DT>()), "range-checked requests");
  static_assert(pf_window_start(Z, 0) == -K && pf_window_start(Z, 3) == 3 * 512 * S - K, "the plan's window grid");
  bool carried = false;        // ka, kb and pf hold this block's window
  // the next window's new pairs, issued on every block (not TAIL: from a window start clamped
  // into the frame, values unused when the next window is not inside it; TAIL: of no bytes
  // after a run's last block): unconditional call sites, so the wait before their use counts
  // only what was issued after them.
  // They are requested in groups at up to five points of the block (fc_prefetch_plan.h) and not
  // in one burst at its head: a wave's 13 requests back to back wait on the memory pipeline's
  // back-pressure wherever they stand (~2,100 cycles of a block when all follow pass C, the
  // stamps of profiles/r09fcpf), 4 + 4 + 5 mostly do not, and the registers of the next window
  // fill as the block goes, which is the room in which fc_hold keeps the whole filter table
  // (cfg2: -2.7 % per step at the hold of before, -3.9 % with it).  The scheduling barriers
  // keep each group where it is written (the compiler otherwise merges the groups of the head
  // and of pass A into one burst).  Zoom 2, complex64: the first FC_PF1 pairs at the head and
  // the rest after pass C, whose 32 values and 16 table pairs leave no room for all 15.
  static_assert(kPfC64 == kInC64 && kPfC32H == kInC32H && kPfCU8 == kInCU8 && kPfF32R == kInF32R, "formats");
  static_assert(pf_step(Z) == S && pf_valid(Z, DT, FLIP), "the plan requests each new pair once");
  constexpr bool PIN = Z != 2 && pf_count(Z, DT, FLIP, kPfHead) != S;
  uint32_t pvo = TAIL ? (uint32_t)pf_lane_off(t, ebytes<DT>()) : 0;
  [[maybe_unused]] const char *const xfr = (const char *)in.p + f * in.stride * ebytes<DT>();  // the frame
  [[maybe_unused]] const char *nw = xfr;  // TAIL: the next window's first byte, the frame's bytes from there
  [[maybe_unused]] int nleft = 0;
  auto pf_group = [&](auto point) {
    constexpr int g = decltype(point)::value;
    constexpr int first = pf_first(Z, DT, FLIP, g), n = pf_count(Z, DT, FLIP, g);
    if constexpr (n > 0 && !(FC_KO & 1)) {
      if constexpr (PIN) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = first; i < first + n; ++i) {
        if constexpr (TAIL) pf[i] = load_pair_r<DT>(nw, nleft, pvo, KEEP + i);
        else pf[i] = load_pair_b<DT, FLIP>(xrs, pvo, KEEP + i);
      }
      if constexpr (PIN) __builtin_amdgcn_sched_barrier(0);
    }
  };
#define FC_PF_AT(point) pf_group(std::integral_constant<int, point>{})
  auto issue_pf = [&](int b) {
    if constexpr (TAIL) {
      const bool more = b + 1 < b1;  // wstart(b + 1) >= 0: b + 1 >= 1
      carried = more;
      const int64_t sn = wstart(b + 1);
      nw = xfr + sn * ebytes<DT>();
      nleft = pf_left_bytes(L, sn, ebytes<DT>(), more);
    } else {
      carried = b + 1 < b1 && inside(b + 1);
      int64_t sn = wstart(b + 1);
      sn = sn < 0 ? 0 : (sn > L - kN ? L - kN : sn);
      pvo = pair_vo<DT, FLIP>(L, sn, t);
    }
    FC_PF_AT(kPfHead);
  };
  for (int b = b0; b < b1; ++b) {
    v2f xa[16], xb[16];
    // this block's lo[Z m0]: a uniform address behind a restrict pointer, so a scalar load, off
    // the vector-memory counter
    const int64_t m0 = (int64_t)P * b;
    const v2f lob = lor[Z * m0];
    {
      const int64_t s = wstart(b);
      if (FC_KO & 1) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          xa[i] = v2f{(float)(t + i), 1.f};
          xb[i] = v2f{1.f, (float)(t - i)};
        }
      } else if (carried) {
#pragma unroll
        for (int i = 0; i < KEEP; ++i) {
          xa[i] = ka[i];
          xb[i] = kb[i];
        }
#pragma unroll
        for (int i = 0; i < S; ++i) cvt_pair<DT, FLIP>(pf[i], xa[KEEP + i], xb[KEEP + i]);
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          if constexpr (TAIL) {
            const int n = (int)s + 2 * t + 512 * i;
            xa[i] = load_sample32<DT>(xrs, (int)L, n);
            xb[i] = load_sample32<DT>(xrs, (int)L, n + 1);
          } else {
            const int64_t n = s + 2 * t + 512 * i;
            xa[i] = load_sample<DT, FLIP>(xrs, L, n);
            xb[i] = load_sample<DT, FLIP>(xrs, L, n + 1);
          }
        }
        // A run's first and a frame's end blocks only.  Waiting here leaves nothing of this
        // branch pending where it joins the carried one: without it the carried branch waits
        // (vmcnt down to 0) for these loads that never ran, which drains the previous block's
        // output stores on every block.  vmcnt 0, expcnt and lgkmcnt at their maxima.
        if (!FC_HEAD_DRAIN) __builtin_amdgcn_s_waitcnt(0x0f70);
      }
#pragma unroll
      for (int i = 0; i < KEEP; ++i) {
        ka[i] = xa[S + i];
        kb[i] = xb[S + i];
      }
      issue_pf(b);
    }
    // pass A: DFT16 over i -> k1, twiddle W_M^(j0 k1), to LDS at ((M / 16) k1 + j0, r)
    dft<16>(xa);
    dft<16>(xb);
    apply_powers2(xa, xb, bA);
#pragma unroll
    for (int k = 0; k < 16; ++k) *(LP4)(bl + aA + 544 * k) = cat(xa[k], xb[k]);
    FC_PF_AT(kPfAfterA);
    __syncthreads();
    // pass B: ((M / 16) k1 + j1 + (M / 256) i2) -> DFT16 over i2 -> k2, twiddle
    // W_(M / 16)^(j1 k2), in place
    {
      v2f ya[16], yb[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const v4f w = *(LP4)(bl + aB + 34 * i);
        ya[i] = lo2(w);
        yb[i] = hi2(w);
      }
      dft<16>(ya);
      dft<16>(yb);
      apply_powers2(ya, yb, bB);
#pragma unroll
      for (int k = 0; k < 16; ++k) *(LP4)(bl + aB + 34 * k) = cat(ya[k], yb[k]);
    }
    FC_PF_AT(kPfAfterB);
    __syncthreads();
    // pass C: ((M / 16) k1 + R1 k2 + j1, r) for all j1 < R1, r < Z -> DFT_R1 over j1 -> k3;
    // Yf = sum_r A_r C; inverse stage 1 (radix R1 over k3 -> b0, twiddle W_M^(-b0 kp)) to
    // (kp + 256 b0)
    {
      v4f cr[16];
#pragma unroll
      for (int j = 0; j < 16; ++j)
        cr[cix(j)] = (FC_KO & 2) ? v4f{1.f, 0.5f, 0.25f, 1.f}
                     : j < HOLD  ? ch[j < HOLD ? j : 0]
                                 : __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(crs, (uint32_t)(16 * t), 4096 * cix(j), 0));
      // one residue pair at a time: its R1 values, DFT each, accumulated into Yf (the whole
      // window's 32 values and C's 32 at once spilled)
      v2f yf[R1];
#pragma unroll
      for (int k = 0; k < R1; ++k) yf[k] = splat(0.f);
#pragma unroll
      for (int rp = 0; rp < Z / 2; ++rp) {
        v2f ea[R1], eb[R1];
#pragma unroll
        for (int j = 0; j < R1; ++j) {
          const v4f w = *(LP4)(bl + aC + 2 * (Z / 2 * j + rp));
          ea[j] = lo2(w);
          eb[j] = hi2(w);
        }
        dft<R1>(ea);
        dft<R1>(eb);
#pragma unroll
        for (int k = 0; k < R1; ++k) {
          const v4f c = cr[Z / 2 * k + rp];
          yf[k] = cmac2(cmac2(yf[k], ea[k], lo2(c)), eb[k], hi2(c));
        }
        if (rp == Z / 4 - 1) FC_PF_AT(kPfMidC);
      }
      idft<R1>(yf);
      pow_tw<R1>(yf, ib0);
      if (ALIAS) __syncthreads();  // every pass-C read done before the inverse array overwrites
#pragma unroll
      for (int q = 0; q < R1; ++q) sl[a1 + Q1 * q] = yf[q];
    }
    __syncthreads();
    FC_PF_AT(kPfAfterC);
    // inverse stages 2..4: radix 4 over the digit at stride S, twiddle W_(4S)^(-b k_low).  They
    // read and write only the elements of their wave's b0 (t >> 6, + 4 h), so the two exchanges
    // between them stay in the wave's registers; stage 5 reads every wave's
#if !FC_INV_LDS
#pragma unroll
    for (int h = 0; h < NB; ++h) {
      v2f v[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) v[a] = sl[a2 + H1 * h + 68 * a];
      idft<4>(v);
      pow_tw<4>(v, ib1);
      xchg_54(v);
      idft<4>(v);
      pow_tw<4>(v, ib2);
      xchg_32(v);
      idft<4>(v);
      pow_tw<4>(v, ib3);
#pragma unroll
      for (int a = 0; a < 4; ++a) sl[a4 + H1 * h + 4 * a] = v[a];
    }
#else
    auto istage = [&](int a0, int st, v2f w) {
#pragma unroll
      for (int h = 0; h < NB; ++h) {
        v2f v[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) v[a] = sl[a0 + H1 * h + st * a];
        idft<4>(v);
        pow_tw<4>(v, w);
#pragma unroll
        for (int a = 0; a < 4; ++a) sl[a0 + H1 * h + st * a] = v[a];
      }
    };
    istage(a2, 68, ib1);
    stage_sync();
    istage(a3, 17, ib2);
    stage_sync();
    istage(a4, 4, ib3);
#endif
    __syncthreads();  // (stage 5 inside the wave, outputs R1 apart: 3.11 -> 3.31 ms, r06fc12)
    // stage 5: radix 4 over a0 -> b4; outputs j = u + (M / 4) b4
    {
      v2f *o = out + f * nd + m0;
      // Zoom 8 and 4 (not cu8) store through a buffer resource over this block's outputs inside the frame,
      // every lane, every time: a lane without a valid output gives an offset past the resource's
      // end, which the range check drops (as the window's loads outside the frame return 0).
      // Four straight-line stores the compiler can count, so its wait for the last prefetched
      // pair at the next block's head leaves them in flight; around stores under a lane
      // condition it waits for everything.
      constexpr bool OBUF = FC_OUT_BUF && Z != 2 && DT != kInCU8;  // the instantiations that spread
      const int64_t left = nd - m0;
      const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc(
          (void *)o, (short)0, OBUF ? 8 * (int)(left < P ? left : P) : 0, kBufFlags);
#pragma unroll
      for (int h = 0; h < NB; ++h) {
        const int i5 = a5(h);
        v2f v[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) v[a] = sl[i5 + a];
        idft<4>(v);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int jm = t + 256 * h + (M / 4) * q - J0;
          if constexpr (OBUF) {
            typedef unsigned u2 __attribute__((ext_vector_type(2)));
            const v2f y = cmul2(v[q], cmul2(lob, lj[h][q]));
            if (!(FC_KO & 4))  // non-temporal, as the pointer stores
              __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2, y), ors,
                                                    jm >= 0 ? 8u * (uint32_t)jm : 0x80000000u, 0, 2);
          } else if (jm >= 0 && jm < P && m0 + jm < nd && !(FC_KO & 4)) {
            if constexpr (LJ) __builtin_nontemporal_store(cmul2(v[q], cmul2(lob, lj[h][q])), o + jm);
            else __builtin_nontemporal_store(cmul2(v[q], cmul2(cmul2(lob, lq[q]), lt[h])), o + jm);
          }
        }
      }
    }
    if (ALIAS) __syncthreads();  // stage-5 reads done before the next window's pass-A stores
  }
#undef FC_PF_AT
}

}  // namespace fc

namespace {

template <int Z>
hipError_t fc_launch(const InDesc &in, const float2 *lo, const float2 *tab, int64_t row_stride, float2 *out,
                     int64_t nd, int frames, hipStream_t st) {
  constexpr int P = fc::Geo<Z>::P;
  const int nb = (int)((nd + P - 1) / P);
  // about two rounds of the chip's 512 resident workgroups: whole frames from 1024 frames per
  // call, below that each frame split into runs of blocks (a run's first window loads in full)
  const int chunks = std::max(1, std::min(nb, (1024 + frames - 1) / frames));
  const int bpc = (nb + chunks - 1) / chunks;
  const dim3 grid((unsigned)((nb + bpc - 1) / bpc), (unsigned)frames);
  const v2f *l = (const v2f *)lo, *tb = (const v2f *)tab;
  v2f *o = (v2f *)out;
#define FC_GO(DT, FL) \
  hipLaunchKernelGGL((fc::fc_decim_kernel<Z, DT, FL>), grid, dim3(256), 0, st, in, l, tb, row_stride, o, nd, bpc)
#define FC_DT(FL)                           \
  do {                                      \
    if (in.dtype == kInC64) FC_GO(kInC64, FL);        \
    else if (in.dtype == kInC32H) FC_GO(kInC32H, FL); \
    else if (in.dtype == kInCU8) FC_GO(kInCU8, FL);   \
    else FC_GO(kInF32R, FL);                          \
  } while (0)
  if (in.flip) FC_DT(1);
  else FC_DT(0);
#undef FC_DT
#undef FC_GO
  return hipGetLastError();
}

}  // namespace

// The zoom-2 instantiations are a translation unit of their own (fc2_kernels.hip includes this
// file with ZFFT_FC_ZOOM2 set): this one keeps zoom 8 and 4, and the two compile side by side.
#ifdef ZFFT_FC_ZOOM2
hipError_t launch_fc2_decim(const InDesc &in, const float2 *lo, const float2 *tab, int64_t row_stride,
                            float2 *out, int64_t nd, int frames, hipStream_t st) {
  return fc_launch<2>(in, lo, tab, row_stride, out, nd, frames, st);
}
#else
hipError_t launch_fc_decim(const InDesc &in, const float2 *lo, const float2 *tab, int64_t row_stride,
                           float2 *out, int64_t nd, int frames, int zoom, hipStream_t st) {
  if (in.len < kFcN || in.len * (int64_t)in_elem_bytes(in.dtype) >= ((int64_t)1 << 31) ||
      (zoom != 8 && zoom != 4 && zoom != 2))
    return hipErrorInvalidValue;
  if (zoom == 8) return fc_launch<8>(in, lo, tab, row_stride, out, nd, frames, st);
  if (zoom == 4) return fc_launch<4>(in, lo, tab, row_stride, out, nd, frames, st);
  return launch_fc2_decim(in, lo, tab, row_stride, out, nd, frames, st);
}
#endif

}  // namespace zfft
