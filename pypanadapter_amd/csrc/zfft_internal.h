// Internal declarations shared by the host files (zfft_plan.cpp, zfft_decim.cpp, zfft_welch.cpp,
// zfft_waterfall.cpp, zfft_persist.cpp, zfft_detect.cpp, zfft_track.cpp, zfft_viewport.cpp,
// zfft_history.cpp, zfft_stream.cpp, zfft_tap.cpp, zfft_chan.cpp, zfft_demod.cpp, zfft_resamp.cpp, zfft_level.cpp, the table builders
// xa_tables.cpp and pc_tables.cpp) and the HIP kernels
// (zfft_kernels.hip, xa_kernels.hip, pc_kernels.hip, fc_kernels.hip, fc2_kernels.hip,
// detect_kernels.hip, detect_local_kernels.hip, track_kernels.hip, view_kernels.hip,
// history_kernels.hip, tap_kernels.hip, chan_kernels.hip, demod_kernels.hip, resamp_kernels.hip, level_kernels.hip).  Not part of the C-ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "zfft_chan_plan.h"    // the channeliser's forms (ChanForm)
#include "zfft_demod_plan.h"   // the demodulator bank's forms (DemodForm, DemodCut)
#include "zfft_resamp_plan.h"  // the resampler bank's forms (ResampForm, ResampCut)
#include "zfft_level_plan.h"   // the level bank's forms (LevelForm, LevelCut)
#include "zfft_detect_plan.h"  // the row detector's forms (DetectForm)
#include "zfft_history_plan.h"  // the row history's quantiser and forms (HistQuant, HistForm)
#include "zfft_tap_plan.h"     // the channel taps' forms and items (TapForm, TapItems)
#include "zfft_track_plan.h"   // the emission tracker's forms and carried records (TrackForm, TrackOpen)
#include "zfft_view_plan.h"    // the viewport's forms (ViewForm)
#include "zfft_welch_plan.h"  // the Welch forms' domains (kMaxLdsFft, kDifMin / kDifMax, ...), WelchSel

struct zfft_emission;  // zfft.h

namespace zfft {

constexpr int kPad = 27;      // sosfiltfilt odd-extension length (3 * ntaps)

// float32 copy of the ↓2 Chebyshev-I SOS cascade (cheby1_q2.h); passed by value as a
// kernel argument so every coefficient lives in SGPRs.
struct Sos32 {
  float b0, b1, b2;  // section 0 numerator; sections 1..3 are exactly [1, 2, 1]
  float a1[4], a2[4];
  float zi[4][2];    // sosfilt_zi
};

Sos32 sos32();

// The caller's frames (the `chunk` of S:2102 / T:1516): sample i of frame f is element
// f * stride + (flip ? len - 1 - i : i) of p, in one of the zfft_config in_dtype formats:
//   0 complex64 (interleaved f32), 1 complex32 (interleaved f16, BASELINE cfg5),
//   2 RTL-SDR interleaved uint8 I,Q, value b/127.5 - 1 (pyrtlsdr packed_bytes_to_iq),
//   3 real float32 (AudioPan's pyaudio paFloat32 stream, S:712-713): I = x, Q = 0.
// flip fuses the sources' np.flip (S:541-543, 459-460) into the stage-0 loads.
enum InDtype { kInC64 = 0, kInC32H = 1, kInCU8 = 2, kInF32R = 3 };
// LO rows (config 4, batched multi-IF): the mixer table holds lo_n rows of lo_stride
// entries; frame f of a call uses row ((lo_first + f) / lo_per) % lo_n (lo_first: the call's
// first frame within a batched host call).  One row (the default) = the plan's f_lo.
struct InDesc {
  const void *p;
  int64_t stride, len;
  int dtype, flip;
  int64_t lo_stride = 0;
  int lo_n = 1, lo_per = 1, lo_first = 0;
};
inline size_t in_elem_bytes(int dtype) { return dtype == kInC64 ? 8 : (dtype == kInC32H || dtype == kInF32R) ? 4 : 2; }

// --- kernels (zfft_kernels.hip); all enqueue on `st`, return hipError_t of the launch ---
// Intermediates use the frame-group-interleaved (FGI) layout: element (f, j) of a
// per-frame sequence of length len lives at ((f/64)*len + j)*64 + f%64 (float2 units);
// buffers hold ngroups = ceil(frames/64) full groups.
struct StageGeom {
  int n;        // stage input length
  int nblk;     // blocks per frame: ceil((n + 27) / block)
  int block;    // S, samples per block (multiple of 16)
  int warmup;   // W, warm-up samples (multiple of 16)
  int ngroups;  // 64-frame groups
  int split = 0;         // stage 0 only: frame groups >= split read a second window set ...
  int64_t alt_off = 0;   // ... starting alt_off samples into each frame (edge windows)
};

hipError_t launch_iir_forward_mix(const InDesc &in, int frames, const float2 *lo,
                                  float2 *yf, const StageGeom &g, hipStream_t st);
hipError_t launch_iir_forward_fgi(const float2 *in, float2 *yf, const StageGeom &g,
                                  hipStream_t st);
hipError_t launch_iir_backward(const float2 *yf, float2 *out, bool natural, int frames,
                               const StageGeom &g, hipStream_t st);

// Fused interior pass pair (commuted stage order, zfft_kernels.hip fused_pass_kernel).
struct FusedGeom {
  int in_len;   // FGI input length (with pads when in_off > 0)
  int in_off;   // 27 when the input is in padded "ext" coordinates, else 0
  int n_mid;    // decimated length ceil((in_len - 2*in_off) / 2) = output length
  int block;    // S in output units (multiple of 16)
  int nblk;     // ceil(n_mid / S)
  int w1, w2;   // warm-up of pass 1 (input rate) and pass 2 (output rate)
  int ngroups;  // 64-frame groups
};

hipError_t launch_fused_pass(const float2 *in, float2 *out, bool desc, bool two, bool nat,
                             const FusedGeom &g, int frames, hipStream_t st);

// "XA" decimation stage (xa_kernels.hip; design model tools/xa_proto.py).  The cascade
// H = N(z)/D(z), N = b0 (1+z^-1)^8, is run as a forward all-pole cascade 1/D(z) at the
// input rate, a 25-tap FIR M = N(z) N(1/z) D(-1/z) evaluated only at the kept (odd)
// positions, and a backward all-pole cascade 1/D2(w), D2(z^2) = D(z) D(-z), at the output
// rate: 8 + 12.5 + 4 multiply-adds per input sample instead of 2 x 17 for two DF2T passes,
// with scipy's pad / steady-state edge rules carried over exactly.  One wave per frame,
// tiles of 64 lanes x B samples (B = 32 or 64), states scanned over lanes in the real modal
// basis of each all-pole cascade (sections slowest pole first, the lower-error fp32 order).
constexpr int kXaLag = 192;          // held-tile outputs corrected by the one-tile lag
constexpr int kXaB = 32;             // lane sub-block: samples per lane and tile
constexpr int kXaRowModes = 2;       // modes scanned inside 16-lane DPP rows (+ one cross-row step)
// Scan levels of mode j for lane sub-blocks of B forward samples (B/2 backward): mode j
// needs |lambda_j|^(S 2^levels) < 1e-9 (radii .935 .808 .682 .587, the backward poles
// squared at half the steps); checked when the tables are built.  Modes 0, 1 scan inside
// 16-lane rows (DPP row shifts, <= 4 levels) and then add the adjacent row's end lane;
// modes 2, 3 take one whole-wave shift (1 level).
__host__ __device__ constexpr int xa_levels(int B, int j) {
  return B == 32 ? (j == 0 ? 4 : j == 1 ? 2 : 1) : (j == 0 ? 3 : 1);
}
struct XaPass {                      // one all-pole cascade, DF-I state (y[t-1], y[t-2]) per section
  float a1[4], a2[4];                // y = x - a1 y[t-1] - a2 y[t-2], cascade order
  float ti[8][8];                    // T^-1: state -> real modal (block lower triangular)
  float t[8][8];                     // T: real modal -> state (block lower triangular)
  float ss[8];                       // modal steady state per unit constant input
  float pS[4][2];                    // lambda_j^S (one lane sub-block of S steps)
  float scan[4][4][2];               // lambda_j^(S 2^d), scan level d
  // modes 0, 1 cross the 16-lane DPP rows once: weight lambda_j^(S dist) of the adjacent
  // row's end lane for lane-in-row i (dist = i + 1 forward, 16 - i backward): c0 s0 c1 s1
  alignas(16) float xr[16][4];
};
struct XaTab {
  XaPass f, b;                       // forward (full rate, S = B), backward (S = B/2)
  float m25[25];                     // M on v[j-8 .. j+16]
  float mp17[17];                    // N(1/z) D(-1/z) on f[j .. j+16] (frame-end form)
  float n9[9];                       // N on v[s .. s-8] (f = N v, frame-end form)
  float mp_sum;                      // h per unit constant f (backward steady input)
  float vss;                         // forward cascade output per unit constant input
  float pad_[2];
  alignas(16) float lag[kXaLag][8];  // backward C A2^d T: held output d steps below the top
  // forward zero-input responses (the exact entering state's part, added after the zero-state
  // pass instead of a second pass): C A^t T for the B own samples, and their images through
  // the FIR -- on this lane's K outputs (gown) and on its share of the next lane's 12 (gnb)
  alignas(16) float fcat[kXaB][8];
  alignas(16) float gown[kXaB / 2][8];
  alignas(16) float gnb[12][8];
};

bool xa_build_tables(XaTab &X, int B);  // xa_tables.cpp; false: scan levels too shallow for the poles
hipError_t launch_xa_stage(const InDesc &in, int n, const float2 *lo, bool mix,
                           float2 *out, int frames, const XaTab *tab, hipStream_t st);

// "PC" (polyphase cascade) decimator for zoom 8 (pc_kernels.hip, host tables pc_tables.cpp,
// design model tools/pc_model.py).  The interior of the three zero-phase stages is, exactly,
//   y1 = (g0 * x)|2, y2 = (g1 * y1)|2        FIRs (33, 49 taps): every all-pole factor of
//                                            stages 0-1 moved to the output rate (polyphase)
//   z2 = S(v) S(1/v) y2                      the two slowest sections of stage 2 at their own
//                                            rate (fp32 conditioning), zero-phase
//   u3 = (g2 * z2)|2                         FIR (57 taps)
//   out = A(w) A(1/w) u3                     10 sections at the output rate (radius <= .765)
// on the zero-extended frame; the frame ends (odd extension, sosfilt_zi states) add a
// low-rank linear map of the first / last input samples onto the first / last outputs.
// K1 = the two FIRs (independent tiles) -> y2 in device memory; K2 = the rest (independent
// tiles with warm-up halos); K3 = the edge maps.  KW ("walk") = K1 + K2 in one launch, one
// workgroup per frame walking its tiles in order: y2 stays in LDS, the causal own-rate
// sections carry their state from tile to tile (no warm-up halo), the anticausal ones warm
// up over the next tile's first 1024 own-rate samples (the output tile lags the FIR tile).
constexpr int kPcStages = 3;              // zoom 8 only
constexpr int kPcQ0 = -16;                // first y2 index of the model's support
constexpr int kPcK1Q = 992;               // y2 outputs per K1 tile
constexpr int kPcK1In = 4128;             // input samples per K1 tile (from 4 q_s - 64)
constexpr int kPcK2M = 2048;              // outputs per K2 tile
constexpr int kPcK2Span = 5376;           // y2 samples per K2 tile: 256 thread blocks of 21
constexpr int kPcK2Left = 560;            // span starts at 2 m0 - 560
constexpr int kPcOwnBlk = 21;             // own-rate samples per thread
constexpr int kPcApBlk = 10;              // output-rate samples per lane (each wave a quarter)
constexpr int kPcApHalo = 64;             // output-rate warm-up per wave (0.765^64 = 3.6e-8:
                                          // the model's fp64 error 5e-8, fp32 2.5e-6 as with 96)
constexpr int kPcG0 = 33, kPcG1 = 49, kPcG2 = 57;
constexpr int kPcOwn = 2, kPcAp = 10;
constexpr int kPcEdgeR = 192, kPcEdgeJ = 1536, kPcEdgeRank = 16;  // edge map capacities
// One second-order all-pole section y[t] = x[t] - a1 y[t-1] - a2 y[t-2] run over lane blocks
// of B samples: state s = (y[t-1], y[t-2]); pw[d] = A^(B 2^d) (row-major 2x2) for the lane
// scan; ct[t] = e0 A^(t+1): output t's response to the entering state.
constexpr int kPcCt = 24;                 // zero-input response rows (>= both block lengths)
struct PcSec {
  float a1, a2, pad_[2];
  float pw[5][4];
  float ct[kPcCt][2];
};
struct PcTab {
  float g0[36], g1[52], g2[60];     // zero-phase FIR taps (centred)
  PcSec own[kPcOwn];                // B = 21 (stage 2's sections 2, 3)
  float own_x[kPcOwn][64][4];       // A^(21 (i + 1)) for lane i (cross-wave scan step)
  PcSec ap[kPcAp];                  // B = 11, slowest first
  PcSec wf[kPcOwn], wb[kPcOwn];     // KW own-rate sections: causal B = 16, anticausal B = 20
  float wf_x[kPcOwn][64][4], wb_x[kPcOwn][64][4];  // A^(B (i + 1)) for those
};
constexpr int kPcWf = 16, kPcWb = 20;    // KW own-rate block lengths (4096 / 5120 samples)
constexpr int kPcWM = 2048;              // KW outputs per tile (= kPcK2M: K2's geometry)
constexpr int kPcWQ = 1024;              // KW y2 per FIR sub-tile (4 per tile)
constexpr int kPcWM0 = -368;             // KW first tile's m0: its FIR tile starts at kPcQ0
__host__ __device__ constexpr int pc_wf_levels(int s) { return s == 0 ? 3 : 5; }
__host__ __device__ constexpr int pc_wb_levels(int s) { return s == 0 ? 3 : 4; }
// Scan levels and correction lengths the kernels are compiled for (checked by the builder).
__host__ __device__ constexpr int pc_own_levels(int s) { return s == 0 ? 3 : 4; }
__host__ __device__ constexpr int pc_ap_levels(int s) {
  return s == 0 ? 3 : s <= 3 ? 2 : s <= 6 ? 1 : 0;
}
__host__ __device__ constexpr int pc_ap_dcut(int s) { return s < 8 ? kPcApBlk : s == 8 ? 8 : 6; }
// Zoom 4 (two stages): the same construction one stage shorter --
//   y1 = (g0 * x)|2                 FIR (33 taps; stage 0's poles moved to the output rate)
//   z1 = S(u) S(1/u) y1             stage 1's two slowest sections at their own rate (= wf, wb)
//   u2 = (g1 * z1)|2                FIR (41 taps: N D2(-u) D{0,1}(-u), zero phase)
//   out = A(w) A(1/w) u2            6 sections at the output rate (D4, D2{0,1}; radius <= .765)
// run by the walk only (pc_walk_kernel<ZOOM = 4>): per tile two FIR sub-tiles of 2048 y1 (the
// input tile of zoom 8's sub-tile) go straight into the own-rate span.
constexpr int kPc4G1 = 41, kPc4Ap = 6;
constexpr int kPc4WM0 = -364;            // first tile's m0: its FIR tile starts at y1 index -8
struct PcTab4 {
  float g0[36], g1[44];             // zero-phase FIR taps (centred)
  PcSec ap[kPc4Ap];                 // B = 11, slowest first
  PcSec wf[kPcOwn], wb[kPcOwn];     // own-rate sections (those of PcTab)
  float wf_x[kPcOwn][64][4], wb_x[kPcOwn][64][4];
  PcSec own[kPcOwn];                // the tiles' own-rate sections (B = 21, those of PcTab)
  float own_x[kPcOwn][64][4];
};
// Zoom 4 as tiles (path 4; few frames per call): K1 = FIR alpha only, y1 (the own-rate signal)
// through device memory from index kPc4Q0 in tiles of 2048; K2 = zoom 8's tail kernel on y1
// with zoom 4's FIR g1 and 6 output-rate sections.
constexpr int kPc4Q0 = -8;               // first y1 index of the model's support
constexpr int kPc4K1M = 2048;            // y1 per K1 tile
int64_t pc4_y1_len(int64_t L);           // y1 entries per frame (from kPc4Q0)
hipError_t launch_pc4_fir(const InDesc &in, const float2 *lo, float2 *y1, int64_t y1_stride,
                          int frames, const PcTab4 *tab, hipStream_t st);
hipError_t launch_pc4_tail(const float2 *y1, int64_t y1_stride, int64_t y1n, float2 *out, int64_t n2,
                           int frames, const PcTab4 *tab, hipStream_t st);
__host__ __device__ constexpr int pc4_ap_levels(int s) { return s == 0 ? 3 : s <= 2 ? 2 : s <= 4 ? 1 : 0; }
__host__ __device__ constexpr int pc4_ap_dcut(int) { return kPcApBlk; }
bool pc_build_tables4(PcTab4 &tab);
// Zoom 2 (one stage) as tiles (the tail kernel on the mixed input, path 4; few frames per call):
// XA's factorisation in the tail kernel's span geometry --
//   v = x / D(z)                    the stage's 4 sections, causal, at the input rate (B = 21)
//   u = (M * v)|2                   M = N(z) N(1/z) D(-1/z): 25 taps, z^-8 .. z^16
//   out = u / D2(1/w)               D2's 4 sections, anticausal, at rate 1/2 (radius <= .874)
// -- each pole once per direction.  The zero-phase form with the two slow sections both ways
// at the input rate (and the other poles at rate 1/2) missed the row gate on a band-edge tone
// (|damp| 1.9e-5); this one is XA's arithmetic.
constexpr int kPc2G = 25, kPc2Ap = 4, kPc2Own = 4;
constexpr int kPc2M0 = -8;                 // power of z of M's first tap
struct PcTab2 {
  float g[28];                      // M_(i + kPc2M0), i < 25
  PcSec own[kPc2Own];               // D's sections at the input rate, B = 21, slowest first
  float own_x[kPc2Own][64][4];      // A^(21 (i + 1)) for lane i (cross-wave step)
  PcSec ap[kPc2Ap];                 // D2's sections at rate 1/2, B = 10, slowest first
};
__host__ __device__ constexpr int pc2_own_levels(int s) { return 4 - s; }
__host__ __device__ constexpr int pc2_ap_levels(int s) { return 4 - s; }
__host__ __device__ constexpr int pc2_ap_dcut(int) { return kPcApBlk; }
bool pc_build_tables2(PcTab2 &tab);
hipError_t launch_pc2_tail(const InDesc &in, const float2 *lo, float2 *out, int64_t n1, int frames,
                           const PcTab2 *tab, hipStream_t st);
// Frame-end maps, out[m] += sum_k U[m][k] (sum_j V[j][k] x[j]) (left: m, j from the start;
// right: from the end), rank r.
struct PcEdge {
  int R = 0, J = 0, r = 0;
  std::vector<float> U, V;         // R x r, J x r (row-major)
};
bool pc_build_tables(PcTab &tab);
// side 0 = frame start, 1 = frame end (depends on L mod 8); _k: K stages (zoom 2^K, L mod 2^K)
bool pc_edge_map(int side, int lmod8, PcEdge &out);
bool pc_edge_map_k(int K, int side, int lmod, PcEdge &out);
int64_t pc_y2_len(int64_t L);      // y2 entries per frame (from kPcQ0)
hipError_t launch_pc_fir(const InDesc &in, const float2 *lo, float2 *y2, int64_t y2_stride,
                         int frames, const PcTab *tab, hipStream_t st);
hipError_t launch_pc_tail(const float2 *y2, int64_t y2_stride, float2 *out, int64_t n3,
                          int frames, const PcTab *tab, hipStream_t st);
hipError_t launch_pc_walk(const InDesc &in, const float2 *lo, float2 *out, int64_t n3, int frames,
                          const PcTab *tab, hipStream_t st);
hipError_t launch_pc_walk4(const InDesc &in, const float2 *lo, float2 *out, int64_t n2, int frames,
                           const PcTab4 *tab, hipStream_t st);
// both frame ends in one launch: [0] = start, [1] = end
// the walk's and FC's: a workgroup per few frames and side, one partial sum per lane and rank
// (K3 below, the tile paths': four, so the two round differently)
hipError_t launch_pc_edge_batch(const InDesc &in, const float2 *lo, float2 *out, int64_t n3, int frames,
                                const float *const U[2], const float *const V[2], const int R[2],
                                const int J[2], const int r[2], hipStream_t st);
hipError_t launch_pc_edge(const InDesc &in, const float2 *lo, float2 *out, int64_t n3, int frames,
                          const float *const U[2], const float *const V[2], const int R[2],
                          const int J[2], const int r[2], hipStream_t st);
// FC (fc_kernels.hip, paths 6 and 7): the zoom-8 model G as a truncated FIR (|k| <= kFcK) applied by
// overlap-save FFT convolution in 8192-sample windows advancing 512 kFcStep samples (kFcP
// outputs); the ↓8 is an alias sum in frequency fused with the filter, the LO mix is the
// filter's modulation.  The table: W_1024^k (k < 1024), then kFcRow entries per LO row.
#ifndef FC_STEP
#define FC_STEP 13  // K = 768 (tail 1.0e-6 of sum |g|; 12 = K 1024, 1.4e-8: 5.5 % slower, r06fc6)
#endif
constexpr int kFcN = 8192, kFcStep = FC_STEP;
constexpr int kFcK = (kFcN - 512 * kFcStep) / 2;   // 768
constexpr int kFcP = 64 * kFcStep;                 // 832
// Zoom 4 (cfg1): four residues of 2048 points, the zoom-4 model truncated at |k| <= 512 (tail
// 1.4e-8 of sum |g|), windows advancing 7168 samples (1792 outputs).
constexpr int kFc4Step = 14;
constexpr int kFc4K = (kFcN - 512 * kFc4Step) / 2;  // 512
constexpr int kFc4P = 512 * kFc4Step / 4;          // 1792
// Zoom 2 (path 7): two residues of 4096 points, the one-stage model truncated at |k| <= 256 (tail
// 1.4e-8 of sum |g|), windows advancing 7680 samples (3840 outputs).
constexpr int kFc2Step = 15;
constexpr int kFc2K = (kFcN - 512 * kFc2Step) / 2;  // 256
constexpr int kFc2P = 512 * kFc2Step / 2;          // 3840
constexpr int kFcRow = kFcN;  // C[k][r] per LO row, v4f pairs [(zoom / 2) k3 + r / 2][t] (r, r+1)
// C for zoom 8, 4 or 2 and LO frequency ratio f_lo / fs into row (kFcRow entries); false if the
// model is unavailable.  unit_lo: without the 1 / sqrt 2 that pairs with the LO table's sqrt 2
// (the FC tails of zoom >= 16 run on a unit LO table).
bool fc_build_row(int zoom, double lo_ratio, float2 *row, bool unit_lo = false);
void fc_build_twiddles(int M, float2 *tw);         // W_M^k, k < M (M = kFcN / zoom)
// zoom 8, 4 or 2; lo: the LO table of the frames (lo[0] real: sqrt 2, or 1 with a unit_lo row)
hipError_t launch_fc_decim(const InDesc &in, const float2 *lo, const float2 *tab, int64_t row_stride,
                           float2 *out, int64_t nd, int frames, int zoom, hipStream_t st);
// zoom 2 (fc2_kernels.hip; launch_fc_decim checks the frame and calls it)
hipError_t launch_fc2_decim(const InDesc &in, const float2 *lo, const float2 *tab, int64_t row_stride,
                            float2 *out, int64_t nd, int frames, hipStream_t st);

struct WelchGeom {
  int n_fft, log2n;
  int n_win;
  int nperseg, step, nseg;
  float scale;  // 1 / (fs * sum(w^2) * nseg)
  // one-sided (real input at zoom 1, scipy's rfft branch): bins 0..N/2,
  // doubled except 0 and N/2, then the reference's fftshift of those N/2+1 bins and its
  // [N/2 - W/2, N/2 + W/2) slice -- row_len = that slice's length, from row_a
  int onesided = 0, row_a = 0, row_len = 0;
  // four-step only: the column pass leaves per-column-group partial sums of each segment and
  // the row pass subtracts mean * FFT(window) after the transform (nperseg == n_fft)
  int fused_mean = 0;
  // in-place DIF only: each frame's segments split over `split` workgroups (few frames per
  // call), their linear partial PSDs in parts[(f split + part) n_win + j], summed in part
  // order and converted to dB by a second launch (split 1: the row directly)
  int split = 1;
  float *parts = nullptr;
};
// Fused mean lines (zfft_plan_segments_per_line; the in-place DIF kernel only), grp >= 1: the
// frame's rows are lines = ceil(nseg / grp) lines of grp segments, rows[(f lines + r) n_win + j];
// WelchGeom::scale is then 1 / (fs sum(w^2) grp), scale_tail the same with the last line's
// segment count, and WelchGeom::split counts parts of whole lines, each written by its own
// workgroup (parts unused).  A kernel argument of its own, after the others: WelchGeom and the
// argument layout of the mean and SEG forms stay as they were.
struct WelchLines {
  int grp = 0, lines = 1;
  float scale_tail = 0.f;
};

// segs (median / max detectors, zfft_plan_average): instead of the dB rows, every segment's
// scaled linear bins into rows[(f nseg + s) n_win + j] (g.scale then without 1/nseg; the split
// form writes them at their absolute s and needs neither g.parts nor a second launch).
// g.split is welch_split's (zfft_welch_plan.h).
hipError_t launch_welch_rows(const float2 *x, int64_t len, const float *win, const float2 *tw,
                             const WelchGeom &g, float *rows, int frames, hipStream_t st,
                             bool segs = false, const WelchLines &ln = WelchLines());

// Four-step Welch for N = N1 * 256, 16 <= N1 <= 256: means (frames*nseg), z (frames*nseg*N)
// workspaces; tws = W_256^m (256) ++ W_N1^m (N1).  seg_out: launch_welch_rows' segs.
hipError_t launch_welch4(const float2 *x, int64_t len, const float *win, const float2 *tw,
                         const float2 *tws, const float2 *winf, const WelchGeom &g, float2 *means,
                         float2 *z, float *rows, int frames, hipStream_t st, bool seg_out = false);

// The detector over a frame's segments: rows[f n_win + j] = 20 log10(median_s / bias) (mode 1,
// numpy's median; inv_bias = 1 / median_bias(nseg)) or 20 log10(max_s) (mode 2) of
// seg[(f nseg + s) n_win + j], j < row_len.
struct WelchSelect {
  int nseg, n_win, row_len;
  int mode;
  float inv_bias;
  int jblocks = 0;  // (set by the launch) workgroups per frame
  // lines (zfft_plan_segments_per_line), grp >= 1: `lines` = ceil(nseg / grp) rows per frame,
  // rows[(f lines + r) n_win + j] the detector over segments [r grp, min(nseg, (r + 1) grp)) of
  // frame f; inv_bias_tail is inv_bias for a shorter last line.  mode 0 (mean) exists here only:
  // inv_bias / inv_bias_tail are then 1 / (the line's segment count).
  int grp = 0, lines = 1;
  float inv_bias_tail = 1.f;
};
// form: how the keys are held (choose_welch's; refused where it does not fit g).
hipError_t launch_welch_select(const float *seg, WelchSelect g, WelchSel form, float *rows, int frames,
                               hipStream_t st);

hipError_t launch_waterfall_init(float *ring, int H, int W, hipStream_t st);
hipError_t launch_waterfall_push(float *ring, int H, int W, const float *rows,
                                 int64_t row_stride, int count, int64_t off0, int scroll,
                                 hipStream_t st);
hipError_t launch_waterfall_read(const float *ring, int H, int W, int64_t off, float *img,
                                 hipStream_t st);
// waterfall rendering: RGBA8 pixels of the ring in read order
// one row (host-visible `row`, or null: none) pushed and the image emitted in one launch:
// RGBA8 through `lut` (f64 false) or float64 (f64 true) into `out` (H*W pixels)
hipError_t launch_waterfall_push_emit(float *ring, int H, int W, int64_t off0, int scroll,
                                      const float *row, const void *lut, double lo, double scale,
                                      void *out, bool f64, hipStream_t st);
hipError_t launch_waterfall_render(const float *ring, int H, int W, int64_t off, const void *lut,
                                   double lo, double scale, void *out, hipStream_t st);
// autolevel order statistics of the pixels < 0: top-16-bit key histogram (65536 bins), then
// the low-16-bit histograms inside nbins (<= 4) chosen top bins
hipError_t launch_autolevel_hist_hi(const float *ring, int64_t n, unsigned *hist, hipStream_t st);
hipError_t launch_autolevel_hist_lo(const float *ring, int64_t n, const unsigned *bins, int nbins,
                                    unsigned *hist, hipStream_t st);
// Persistence spectrum (zfft.h's binning rule): hist[level * n_win + j] += the number of rows
// r < count whose value rows[r * row_stride + j], j < row_len, falls in `level`.  One launch:
// a workgroup owns 64 consecutive columns and one of `slices` row slices (persist_slices),
// counts in LDS and adds its non-zero cells to hist at the end.
struct PersistGeom {
  int n_win, row_len, levels;
  float lo, inv;
  int slices = 0, slice_rows = 0;  // (set by the launch)
};
int persist_slices(int count, int row_len);
hipError_t launch_persist_hist(const float *rows, int64_t row_stride, int count, PersistGeom g,
                               unsigned *hist, hipStream_t st);
// hist[i] = floor((double)hist[i] * keep), i < n
hipError_t launch_persist_decay(unsigned *hist, int64_t n, double keep, hipStream_t st);
// Row detector (zfft.h's rule; detect_kernels.hip): per row r < count of rows[r * row_stride + j],
// j < row_len, the floor, the number of kept runs and the first max_per_row records, and occ[j]
// += 1 for every column of a kept run.  `form` is choose_detect's (refused where it does not
// hold row_len); events 16-byte aligned.
struct DetectGeom {
  int n_win, row_len;
  double q;        // the floor's quantile
  float thr_add;   // (float)threshold_db
  int min_width, max_per_row;
};
hipError_t launch_detect_rows(const float *rows, int64_t row_stride, int count, const DetectGeom &g,
                              const DetectForm &form, float *floor_out, int32_t *found_out,
                              zfft_emission *events, unsigned *occ, hipStream_t st,
                              const float *col_floor = nullptr);
// col_floor (zfft_plan_detect_local): count rows of stride g.n_win; column j of row r is then on
// against col_floor[r * g.n_win + j] + thr_add instead of the row's floor (which floor_out still
// gets).
// The local floors (zfft.h's rule of zfft_plan_detect_local; detect_local_kernels.hip):
// floors[r * floor_stride + j], r < count, j < row_len, the value of rank floor(q (m - 1)) among
// the m finite values of rows[r * row_stride + c], guard < |c - j| <= guard + half_window,
// 0 <= c < row_len; NaN where m == 0.  Columns at or beyond row_len are left untouched.  `form`
// is choose_detect_local's for these arguments.
hipError_t launch_detect_floors(const float *rows, int64_t row_stride, int count, int row_len, int half_window,
                                int guard, double q, const DetectLocalForm &form, float *floors, int64_t floor_stride,
                                hipStream_t st);
// Emission tracker (zfft.h's rule of zfft_plan_track; track_kernels.hip): one pass of R rows,
// found / events the pass's first row's, t0 its row number.  The carried state (fr_*: the last
// G = gap + 1 rows given, row-major, K slots each; open_tab; ctr; store, a ring read from `head`)
// and the pass's scratch (per node of the (R + G) * K: parent, the candidates c_* and the aggregates
// a_*, these zeroed before the first step; per local row: rowcnt, rowoff).  The steps 0 .. kTrackSteps - 1 run in
// order on one stream; kTrackStepNames[step] is the launch's name.
struct TrackArgs {
  int K, G, slack, min_rows, max_tracks;
  int R, chunk_rows, chunks;
  int64_t t0;
  uint32_t head;
  const int32_t *found;
  const zfft_emission *events;
  zfft_emission *fr_ev;
  int32_t *fr_found;
  uint32_t *fr_parent;
  TrackOpen *open_tab;
  TrackCounters *ctr;
  zfft_track *store;
  uint32_t *parent;
  uint64_t *a_name, *a_last, *a_cells, *a_runs, *a_prow;
  uint32_t *a_colf, *a_coll, *a_pkey, *a_pcol;
  // per candidate (a chunk's root, a seeded frontier node): the peak of its part, plain values
  uint64_t *c_prow;
  uint32_t *c_pkey, *c_pcol;
  int32_t *rowcnt, *rowoff;  // per local row its reported tracks; per kTrackThreads rows their store offset
};
constexpr int kTrackSteps = 9;
extern const char *const kTrackStepNames[kTrackSteps];
hipError_t launch_track_step(int step, const TrackArgs &a, hipStream_t st);
// Closes every open track as it stands and empties the frontier (needs the carried state only).
hipError_t launch_track_flush(const TrackArgs &a, hipStream_t st);
// Display viewport (zfft.h's rule; view_kernels.hip): one push of `count` rows of stride n_win
// into the ring of H lines of `width` pixels, pixel x the columns [col0 + x span / width,
// col0 + (x + 1) span / width).  The push continues a group of `pending` rows (its accumulator
// in `pend`: width floats, or width float64 linear sums for det 2) and completes ncomp =
// (pending + count) / m lines, line r into the slot that is image row H - 1 (scroll +1) or 0
// (scroll -1) after off0 has advanced by (r + 1) scroll.  traces: last,
// max_hold, min_hold, width floats each.  `f` is choose_view's for the push (refused otherwise).
struct ViewGeom {
  int n_win, col0, span, width;
  int det, m;               // zfft_view_detector, rows_per_line
  int H, off0, scroll;
  int count, pending, ncomp;
  int direct;               // view_direct: launch_view_lines alone does the whole push
};
// One workgroup per tile and no partial group in the push: the lines kernel updates the hold
// traces itself and there is no finishing launch.
bool view_direct(const ViewGeom &g, const ViewForm &f);
size_t view_scratch_bytes(const ViewForm &f, int width);
hipError_t launch_view_lines(const float *rows, const ViewGeom &g, const ViewForm &f, float *ring, float *traces,
                             void *scratch, size_t scratch_bytes, hipStream_t st);
hipError_t launch_view_finish(const ViewGeom &g, const ViewForm &f, float *ring, float *traces, void *pend,
                              const void *scratch, size_t scratch_bytes, hipStream_t st);
hipError_t launch_view_fill(float *p, int64_t n, float v, hipStream_t st);
// Row history (zfft.h's rule; history_kernels.hip): a ring of `cap` stored rows of `stride`
// elements (hist_stride(n): float32, uint16 or uint8 codes by q.format), row R of the store's
// numbering in slot R mod cap, its first n elements the row's columns and the rest padding.
struct HistStore {
  void *data;
  int64_t cap, stride;
  int n;
  HistQuant q;
};
// rows[i * n_win + j], j < n, i < count, into the slots of the rows row0 + i (one launch; the
// slots may wrap the ring's end; count <= cap).
hipError_t launch_history_pack(const float *rows, int n_win, int count, int64_t row0, const HistStore &s,
                               hipStream_t st);
// the stored rows row0 + i, i < count, unpacked into rows[i * n_win + j], j < n
hipError_t launch_history_unpack(const HistStore &s, int64_t row0, int count, int n_win, float *rows, hipStream_t st);
// A view (zfft_history_window): line L < lines of img (lines x width) over the rows [first + L m,
// first + (L + 1) m), all NaN unless those lie in [oldest, seen).  `f` is choose_history's for
// the window (refused otherwise); a sliced form leaves partials in `scratch` and needs
// launch_history_finish.
struct HistGeom {
  int64_t first, oldest, seen;
  int col0, span, width;
  int det, m, lines;
};
size_t history_scratch_bytes(const HistForm &f, int width);
hipError_t launch_history_view(const HistStore &s, const HistGeom &g, const HistForm &f, float *img, void *scratch,
                               size_t scratch_bytes, hipStream_t st);
hipError_t launch_history_finish(const HistStore &s, const HistGeom &g, const HistForm &f, float *img,
                                 const void *scratch, size_t scratch_bytes, hipStream_t st);
// Channel taps (zfft.h's rule of zfft_plan_taps; tap_kernels.hip): one push of n samples of `in`
// (one of the InDtype formats, not flipped) as choose_tap cut it.  tab holds a row of max_len
// entries c[k] per slot; carry_old the max_len - 1 samples before the push, carry_new those before
// the next (two buffers: the first workgroups read the one while the last write the other); out
// the items' outputs back to back.  in, out and the carries do not overlap.
hipError_t launch_tap_push(const void *in, int dtype, int64_t n, int max_len, const TapForm &f, const TapItems &items,
                           const float2 *tab, const float2 *carry_old, float2 *carry_new, float2 *out,
                           hipStream_t st);
// Channeliser (zfft.h's rule of zfft_plan_chan; chan_kernels.hip): one push of n samples of `in`
// (one of the InDtype formats, not flipped) as choose_chan cut it for K kept channels from c_first.
// h holds the M P prototype taps, tw chan_twiddles(M); carry_old the M P - 1 samples before the
// push, carry_new those before the next; out[step * K + i].  in, out and the carries do not overlap.
hipError_t launch_chan_push(const void *in, int dtype, int64_t n, int M, int P, int D, int c_first, int K,
                            const ChanForm &f, const float *h, const float2 *tw, const float2 *carry_old,
                            float2 *carry_new, float2 *out, hipStream_t st);
// Demodulator bank (zfft.h's rule of zfft_plan_demod; demod_kernels.hip): one push of `steps` steps
// of K complex64 streams at x[step * step_stride + stream * stream_stride], count n0 at the first,
// as choose_demod and demod_cut tiled it.  taps holds the Ta audio taps, par K (mode, bfo_word)
// pairs; carry_old the Ta steps before the push ([row * K + stream]), carry_new those before the
// next; out[j * K + stream].  x, out and the carries do not overlap.
hipError_t launch_demod_push(const float2 *x, int64_t steps, int64_t step_stride, int64_t stream_stride, uint64_t n0,
                             int K, int Ta, int Da, const DemodForm &f, const DemodCut &c, const float *taps,
                             const uint32_t *par, const float2 *carry_old, float2 *carry_new, float *out,
                             hipStream_t st);
// par[s_first .. s_first + s_count) = (mode, word), in stream order.
hipError_t launch_demod_mode(uint32_t *par, int s_first, int s_count, uint32_t mode, uint32_t word, hipStream_t st);
// Resampler bank (zfft.h's rule of zfft_plan_resamp; resamp_kernels.hip): one push of `steps` steps of
// f.K float32 lanes at x[step * step_stride + lane], as choose_resamp and resamp_cut tiled it.  hp
// holds the table phase-major, hp[phase * T + k] = h[k L + phase]; carry_old the T - 1 steps before
// the push ([row * K + lane]), carry_new those before the next; out[j * K + lane], float32 or (S16)
// int16 of the product with `scale`.  x, out and the carries do not overlap.
hipError_t launch_resamp_push(const float *x, int64_t steps, int64_t step_stride, const ResampForm &f, const ResampCut &c,
                              int format, float scale, const float *hp, const float *carry_old, float *carry_new,
                              void *out, hipStream_t st);
// Level bank (zfft.h's rule of zfft_plan_level; level_kernels.hip): the three launches of one push,
// as choose_level and level_cut tiled it.  A carry holds (2 B - 1) K unemitted steps, K running
// peaks and (H + 2) K block peaks; pk the push's c.npk x K peaks, gk its c.nq x K block gains.
// peaks: the key's blocks into pk and carry_new's running peak.  gains (only where c.outs > 0):
// pk into gk with par = {target, gmax, floor, squelch}.  apply: out[j * K + lane] and the rest of
// carry_new.  x, key, out, the carries, pk and gk do not overlap.
hipError_t launch_level_peaks(const float *key, int64_t key_stride, const LevelForm &f, const LevelCut &c,
                              const float *carry_old, float *carry_new, float *pk, hipStream_t st);
hipError_t launch_level_gains(const LevelForm &f, const LevelCut &c, const float par[4], const float *pk, float *gk,
                              hipStream_t st);
hipError_t launch_level_apply(const float *x, int64_t x_stride, const LevelForm &f, const LevelCut &c, const float *carry_old,
                              float *carry_new, const float *pk, const float *gk, float *out, hipStream_t st);
// out[f][i] = in(f, i) (* lo[i] when lo) as complex64, natural layout, frames x len.
hipError_t launch_fill_c64(float2 *out, int64_t n, float re, float im, hipStream_t st);
hipError_t launch_ingest(const InDesc &in, const float2 *lo, float2 *out, int frames,
                         hipStream_t st);

// --- host helpers ---
void set_error(const std::string &msg);
bool window_kind_native(int kind);
bool make_window(int kind, const double *param, int M, std::vector<double> &out);

}  // namespace zfft
