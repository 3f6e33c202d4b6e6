// zfft_decim.cpp -- the decimator of libzfft.so: the LO / PC / FC tables of a plan and one
// runner per schedule (zfft_schedule.h); run_decimator launches what choose_schedule names.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <new>
#include <vector>

#include "pc_edge_maps.h"
#include "zfft.h"
#include "zfft_plan.h"
#include "zfft_schedule.h"

namespace zfft {

static_assert(kSchedPcStages == kPcStages && kSchedFcMinL == kFcN, "zfft_schedule.h mirrors the kernels' geometry");

std::vector<int64_t> stage_lengths(int64_t L, int K) {
  std::vector<int64_t> n{L};
  for (int k = 0; k < K; ++k) n.push_back((n.back() + 1) / 2);
  return n;
}

namespace {

int choose_block(const zfft_plan *p, int64_t n, int ngroups) {
  if (p->block_override > 0) return (p->block_override + 15) & ~15;
  // Enough waves (one per block of a 64-frame group) to fill 256 CUs many times over;
  // larger blocks amortise the warm-up.  A few frames of <= 2^19 samples (one per call:
  // the reference's use) go down to 256-sample blocks, whose shorter serial runs took one
  // cfg2 frame from 0.48 to 0.38 ms of kernels (cfg5's 2^20-sample frames: no gain).
  const int s_min = n <= ((int64_t)1 << 19) ? 256 : 512;
  int S = 4096;
  while (S > s_min && (int64_t)ngroups * ((n + kPad + S - 1) / S) < 8192) S >>= 1;
  return S;
}

int warmup(const zfft_plan *p) { return p->warm_override > 0 ? (p->warm_override + 15) & ~15 : 192; }

}  // namespace

// LO table: one row of lo_len entries per LO frequency (the plan's f_lo, or the
// zfft_plan_set_lo_frames list), rows lo_len apart.
constexpr size_t kMaxLoBytes = (size_t)4 << 30;  // the LO table, all rows
int ensure_lo(zfft_plan *p, int64_t L) {
  if (p->lo_len >= L) return ZFFT_OK;
  int rc = quiesce(p);
  if (rc) return rc;
  // the XA kernels read lo[lane] for every lane; rows 64-entry aligned
  const int64_t cap = (std::max<int64_t>(L, 64) + 63) & ~(int64_t)63;
  const std::vector<double> freqs = p->lo_freqs.empty() ? std::vector<double>{p->cfg.f_lo} : p->lo_freqs;
  if ((double)cap * (double)freqs.size() * sizeof(float2) > (double)kMaxLoBytes)
    return fail(ZFFT_ENOMEM, "LO table (set_lo_frames rows x frame length x 8 B) over 4 GiB");
  std::vector<float2> h;
  try {
    h.resize(cap * freqs.size());
  } catch (const std::bad_alloc &) {
    return fail(ZFFT_ENOMEM, "LO table host staging allocation failed");
  }
  const double sq2 = std::sqrt(2.0);
  for (size_t k = 0; k < freqs.size(); ++k) {
    const double r = freqs[k] / p->cfg.fs;
    for (int64_t n = 0; n < cap; ++n) {
      // lo[n] = sqrt(2) exp(-2 pi i f_lo n / fs) on integer n (S:2091-2093)
      const double turns = std::fmod((double)n * r, 1.0);
      const double ph = -2.0 * M_PI * turns;
      h[k * cap + n] = make_float2((float)(sq2 * std::cos(ph)), (float)(sq2 * std::sin(ph)));
    }
  }
  hipError_t e = p->lo.ensure(h.size() * sizeof(float2));
  if (e != hipSuccess) return fail(ZFFT_ENOMEM, "LO table allocation failed");
  e = hipMemcpy(p->lo.p, h.data(), h.size() * sizeof(float2), hipMemcpyHostToDevice);
  if (e != hipSuccess) return hip_fail(e, "LO table upload");
  p->lo_len = cap;
  return ZFFT_OK;
}

namespace {

// Exact decimation cascade (reference pass order, odd padding, zi initial conditions) on
// `frames` frames of n[0] samples each at frame stride `stride` (natural layout in; lo points
// at the LO value of the first sample).  Intermediates in FGI layout, the result (last
// stage) in natural layout in *out.
// With split > 0 (a multiple of 64) the frames [split, split + frames) are a second window
// set starting alt_off samples into the same frames; the output then has split + frames rows.
// k0 > 0: stages k0 .. K-1 only, `in` holding stage k0's input (already mixed: lo a unit
// table), e.g. after the PC head.
int run_exact(zfft_plan *p, const InDesc &in, const float2 *lo, int frames,
              const std::vector<int64_t> &n, const float2 **out, hipStream_t st, int split = 0,
              int64_t alt_off = 0, int k0 = 0) {
  const int rows = split > 0 ? split + frames : frames;
  const int ngroups = (rows + 63) / 64;
  const size_t G = (size_t)ngroups * 64;
  hipError_t e = p->yf.ensure(G * (n[k0] + 2 * kPad) * sizeof(float2));
  if (e == hipSuccess) e = p->ping.ensure(G * n[k0 + 1] * sizeof(float2));
  if (e == hipSuccess && p->K > k0 + 1) e = p->pong.ensure(G * n[k0 + 2] * sizeof(float2));
  if (e != hipSuccess) return fail(ZFFT_ENOMEM, "decimator workspace allocation failed");
  const float2 *cur = nullptr;
  for (int k = k0; k < p->K; ++k) {
    StageGeom g;
    g.n = (int)n[k];
    g.block = choose_block(p, n[k], ngroups);
    g.nblk = (int)((n[k] + kPad + g.block - 1) / g.block);
    g.warmup = warmup(p);
    g.ngroups = ngroups;
    g.split = split;
    g.alt_off = alt_off;
    if (k == k0)
      e = launch_iir_forward_mix(in, frames, lo, p->yf.as<float2>(), g, st);
    else
      e = launch_iir_forward_fgi(cur, p->yf.as<float2>(), g, st);
    if (e != hipSuccess) return hip_fail(e, "iir_forward launch");
    mark(p, st, k == 0 ? "exact_forward_mix" : "exact_forward");
    float2 *dst = ((k - k0) & 1) ? p->pong.as<float2>() : p->ping.as<float2>();
    e = launch_iir_backward(p->yf.as<float2>(), dst, k == p->K - 1, rows, g, st);
    if (e != hipSuccess) return hip_fail(e, "iir_backward launch");
    mark(p, st, "exact_backward");
    cur = dst;
  }
  *out = cur;
  return ZFFT_OK;
}

int fused_block(int64_t n_mid, int ngroups) {
  int S = 2048;
  while (S > 256 && (int64_t)ngroups * ((n_mid + S - 1) / S) < 4096) S >>= 1;
  return S;
}

// Interior in commuted pass order with fused same-direction pass pairs, edges exact:
//   [C0] [A0 A1] [C1 C2] [A2 A3] ... [last pass of stage K-1, decimated, natural layout]
// then the first/last kEdge outputs are replaced by the exact pipeline on prefix/suffix
// windows of the frames (run first, their edge outputs parked in p->edge).
int run_fused(zfft_plan *p, const InDesc &in, int64_t L, int frames,
              const std::vector<int64_t> &n, const float2 **out, hipStream_t st) {
  const int K = p->K;
  const int64_t nK = n[K];
  const int ngroups = (frames + 63) / 64;
  const size_t G = (size_t)ngroups * 64;
  const int64_t P = edge_window(K);
  const int64_t L0 = ((L - P) >> K) << K;  // suffix window start, multiple of 2^K
  // both window sets have length Pw = L - L0 in [P, P + 2^K): the suffix ends at the frame end
  const std::vector<int64_t> npre = stage_lengths(L - L0, K), nsuf = npre;
  // all workspace first (the window runs reuse the interior chain's buffers)
  hipError_t e = p->edge.ensure((size_t)frames * 2 * kEdge * sizeof(float2));
  if (e == hipSuccess) e = p->xk.ensure((size_t)frames * nK * sizeof(float2));
  if (e == hipSuccess) e = p->yf.ensure(G * (L + 2 * kPad) * sizeof(float2));
  if (e == hipSuccess) e = p->ping.ensure(G * n[1] * sizeof(float2));
  if (e == hipSuccess) e = p->pong.ensure(G * n[2] * sizeof(float2));
  if (e != hipSuccess) return fail(ZFFT_ENOMEM, "decimator workspace allocation failed");
  float2 *edge = p->edge.as<float2>();
  // exact edges: one run over prefix windows (rows [0, F)) and suffix windows (rows
  // [Fp, Fp + F), Fp = F rounded up to 64); then prefix cols [0, E) and suffix cols
  // [nsuf_K - E, nsuf_K) -> p->edge [F][2E]
  const int Fp = ngroups * 64;
  const float2 *w;
  int rc = run_exact(p, in, p->lo.as<float2>(), frames, npre, &w, st, Fp, L0);
  if (rc) return rc;
  e = hipMemcpy2DAsync(edge, 2 * kEdge * sizeof(float2), w, npre[K] * sizeof(float2),
                       kEdge * sizeof(float2), frames, hipMemcpyDeviceToDevice, st);
  if (e != hipSuccess) return hip_fail(e, "edge copy");
  e = hipMemcpy2DAsync(edge + kEdge, 2 * kEdge * sizeof(float2),
                       w + (int64_t)Fp * npre[K] + (nsuf[K] - kEdge), npre[K] * sizeof(float2),
                       kEdge * sizeof(float2), frames, hipMemcpyDeviceToDevice, st);
  if (e != hipSuccess) return hip_fail(e, "edge copy");
  mark(p, st, "edge_windows");

  // interior chain
  StageGeom g0;
  g0.n = (int)L;
  g0.block = choose_block(p, L, ngroups);
  g0.nblk = (int)((L + kPad + g0.block - 1) / g0.block);
  g0.warmup = warmup(p);
  g0.ngroups = ngroups;
  e = launch_iir_forward_mix(in, frames, p->lo.as<float2>(), p->yf.as<float2>(), g0, st);
  if (e != hipSuccess) return hip_fail(e, "iir_forward launch");
  mark(p, st, "C0_forward_mix");
  const float2 *cur = p->yf.as<float2>();
  int64_t cur_len = L + 2 * kPad;
  int cur_off = kPad;
  for (int i = 0; i <= K - 1; ++i) {  // kernel i: 2nd pass of stage i (+ 1st of stage i+1)
    const bool two = i < K - 1;
    FusedGeom fg;
    fg.in_len = (int)cur_len;
    fg.in_off = cur_off;
    fg.n_mid = (int)n[i + 1];
    fg.block = fused_block(fg.n_mid, ngroups);
    fg.nblk = (fg.n_mid + fg.block - 1) / fg.block;
    fg.w1 = fg.w2 = warmup(p);
    fg.ngroups = ngroups;
    float2 *dst = !two ? p->xk.as<float2>() : ((i & 1) ? p->pong.as<float2>() : p->ping.as<float2>());
    e = launch_fused_pass(cur, dst, (i & 1) == 0, two, !two, fg, frames, st);
    if (e != hipSuccess) return hip_fail(e, "fused pass launch");
    mark(p, st, two ? ((i & 1) ? "fused_asc_pair" : "fused_desc_pair")
                    : ((i & 1) ? "fused_asc_last" : "fused_desc_last"));
    cur = dst;
    cur_len = n[i + 1];
    cur_off = 0;
  }
  // patch the exact edges into the interior result
  float2 *xk = p->xk.as<float2>();
  e = hipMemcpy2DAsync(xk, nK * sizeof(float2), edge, 2 * kEdge * sizeof(float2),
                       kEdge * sizeof(float2), frames, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess)
    e = hipMemcpy2DAsync(xk + (nK - kEdge), nK * sizeof(float2), edge + kEdge,
                         2 * kEdge * sizeof(float2), kEdge * sizeof(float2), frames,
                         hipMemcpyDeviceToDevice, st);
  if (e != hipSuccess) return hip_fail(e, "edge patch");
  mark(p, st, "edge_patch");
  *out = xk;
  return ZFFT_OK;
}

// XA path: one wave per frame and stage launch, stage outputs in natural layout (ping /
// pong).  Two or three stages per launch through per-frame rings measured slower.
int run_xa(zfft_plan *p, const InDesc &in, int frames, const std::vector<int64_t> &n,
           const float2 **out, hipStream_t st) {
  hipError_t e = p->ping.ensure((size_t)frames * n[1] * sizeof(float2));
  if (e == hipSuccess && p->K > 1) e = p->pong.ensure((size_t)frames * n[2] * sizeof(float2));
  if (e != hipSuccess) return fail(ZFFT_ENOMEM, "decimator workspace allocation failed");
  const float2 *cur = nullptr;
  for (int k = 0; k < p->K; ++k) {
    float2 *dst = (k & 1) ? p->pong.as<float2>() : p->ping.as<float2>();
    const InDesc src = k == 0 ? in : InDesc{cur, n[k], n[k], kInC64, 0};
    e = launch_xa_stage(src, (int)n[k], p->lo.as<float2>(), k == 0, dst, frames,
                        p->xa_tab.as<XaTab>(), st);
    if (e != hipSuccess) return hip_fail(e, "xa_stage launch");
    mark(p, st, k == 0 ? "xa_stage_mix" : "xa_stage");
    cur = dst;
  }
  *out = cur;
  return ZFFT_OK;
}

// Host copy of the PC tables: built once per process (fp64, microseconds); the frame-end maps
// are the constants of pc_edge_maps.h (tools/gen_pc_edge.py).
const PcTab *pc_host_tab() {
  static const std::unique_ptr<PcTab> t = [] {
    std::unique_ptr<PcTab> x(new PcTab());
    if (!pc_build_tables(*x)) x.reset();
    return x;
  }();
  return t.get();
}
const PcTab2 *pc_host_tab2() {
  static const std::unique_ptr<PcTab2> t = [] {
    std::unique_ptr<PcTab2> x(new PcTab2());
    if (!pc_build_tables2(*x)) x.reset();
    return x;
  }();
  return t.get();
}
const PcTab4 *pc_host_tab4() {
  static const std::unique_ptr<PcTab4> t = [] {
    std::unique_ptr<PcTab4> x(new PcTab4());
    if (!pc_build_tables4(*x)) x.reset();
    return x;
  }();
  return t.get();
}

// The frame-end map table of a K-stage PC form (pc_edge_maps.h): 1 + 2^K maps.
static_assert(kPcEdge2Maps == 3 && kPcEdge4Maps == 5 && kPcEdgeMaps == 9, "one start map + 2^K end maps");
const PcEdgeConst *edge_idx(int K) { return K == 1 ? kPcEdge2Idx : K == 2 ? kPcEdge4Idx : kPcEdgeIdx; }

// The PC tables and all frame-end maps, uploaded on the plan's first PC call; nothing is
// uploaded afterwards, so a change of L mod 8 between calls never waits on enqueued work.
int ensure_pc(zfft_plan *p) {
  if (p->pc_tab.p && p->pc_tab4.p && p->pc_tab2.p && p->pc_edge.p) return ZFFT_OK;
  const PcTab *t = pc_host_tab();
  const PcTab4 *t4 = pc_host_tab4();
  const PcTab2 *t2 = pc_host_tab2();
  if (!t || !t4 || !t2) return fail(ZFFT_EINTERNAL, "PC tables: scan depth or correction length too short");
  for (int K = 1; K <= kPcStages; ++K)
    for (int i = 0; i < 1 + (1 << K); ++i) {
      const PcEdgeConst &m = edge_idx(K)[i];
      if (m.r > kPcEdgeRank || m.R > kPcEdgeR || m.R > 256)
        return fail(ZFFT_EINTERNAL, "PC frame-end maps exceed the kernel's capacities");
    }
  hipError_t e = p->pc_tab.ensure(sizeof(PcTab));
  if (e == hipSuccess) e = hipMemcpy(p->pc_tab.p, t, sizeof(PcTab), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = p->pc_tab4.ensure(sizeof(PcTab4));
  if (e == hipSuccess) e = hipMemcpy(p->pc_tab4.p, t4, sizeof(PcTab4), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = p->pc_tab2.ensure(sizeof(PcTab2));
  if (e == hipSuccess) e = hipMemcpy(p->pc_tab2.p, t2, sizeof(PcTab2), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = p->pc_edge.ensure(sizeof(kPcEdgeData));
  if (e == hipSuccess) e = hipMemcpy(p->pc_edge.p, kPcEdgeData, sizeof(kPcEdgeData), hipMemcpyHostToDevice);
  if (e != hipSuccess) return hip_fail(e, "PC table upload");
  return ZFFT_OK;
}

// FC tables for the plan's LO rows and FC's zoom (2, 4 or 8): host fp64 build, fc_build_row; one
// synchronous upload when the LO frequencies change, after the plan's enqueued work.
int ensure_fc(zfft_plan *p, int zoom) {
  const std::vector<double> freqs = p->lo_freqs.empty() ? std::vector<double>{p->cfg.f_lo} : p->lo_freqs;
  std::vector<double> ratios;
  for (double fr : freqs) ratios.push_back(fr / p->cfg.fs);
  if (p->fc_tab.p && p->fc_built == ratios) return ZFFT_OK;  // (ratios is never empty)
  int rc = quiesce(p);
  if (rc) return rc;
  const int M = kFcN / zoom;
  std::vector<float2> h;
  try {
    h.resize(M + ratios.size() * (size_t)kFcRow);
  } catch (const std::bad_alloc &) {
    return fail(ZFFT_ENOMEM, "FC table host staging allocation failed");
  }
  fc_build_twiddles(M, h.data());
  for (size_t k = 0; k < ratios.size(); ++k)
    if (!fc_build_row(zoom, ratios[k], h.data() + M + k * kFcRow))
      return fail(ZFFT_EINTERNAL, "FC table: model response unavailable");
  // from here the old table may be gone (ensure reallocates when it grows) or half written:
  // not built until the upload has succeeded
  p->fc_built.clear();
  hipError_t e = p->fc_tab.ensure(h.size() * sizeof(float2));
  if (e != hipSuccess) return fail(ZFFT_ENOMEM, "FC table allocation failed");
  e = hipMemcpy(p->fc_tab.p, h.data(), h.size() * sizeof(float2), hipMemcpyHostToDevice);
  if (e != hipSuccess) return hip_fail(e, "FC table upload");
  p->fc_built = ratios;
  return ZFFT_OK;
}

// The tables of the FC tails (zoom >= 16, path 7): for launch zoom 8, 4 and 2 the twiddles and
// the row of f_lo = 0 without the LO's 1 / sqrt 2, at fc_tail_off(zoom); built and uploaded once.
size_t fc_tail_off(int zoom) {
  size_t off = 0;
  for (int z = 8; z > zoom; z >>= 1) off += kFcN / z + kFcRow;
  return off;
}
int ensure_fc_tail(zfft_plan *p) {
  if (p->fc_tail_tab.p) return ZFFT_OK;
  std::vector<float2> h;
  try {
    h.resize(fc_tail_off(1));
  } catch (const std::bad_alloc &) {
    return fail(ZFFT_ENOMEM, "FC table host staging allocation failed");
  }
  for (int z = 8; z >= 2; z >>= 1) {
    float2 *t = h.data() + fc_tail_off(z);
    fc_build_twiddles(kFcN / z, t);
    if (!fc_build_row(z, 0.0, t + kFcN / z, true))
      return fail(ZFFT_EINTERNAL, "FC table: model response unavailable");
  }
  DevBuf tab;  // the plan's only once it is whole
  hipError_t e = tab.ensure(h.size() * sizeof(float2));
  if (e != hipSuccess) return fail(ZFFT_ENOMEM, "FC table allocation failed");
  e = hipMemcpy(tab.p, h.data(), h.size() * sizeof(float2), hipMemcpyHostToDevice);
  if (e != hipSuccess) return hip_fail(e, "FC table upload");
  std::swap(p->fc_tail_tab.p, tab.p);
  std::swap(p->fc_tail_tab.cap, tab.cap);
  return ZFFT_OK;
}

// The frame-end maps of a K-stage PC form for frames of L samples, in the plan's device copy
// of pc_edge_maps.h: [0] = frame start (map 0), [1] = frame end (map 1 + L mod 2^K).
struct EdgeMaps {
  const float *U[2], *V[2];
  int R[2], J[2], r[2];
};
EdgeMaps edge_maps(const zfft_plan *p, int K, int64_t L) {
  const PcEdgeConst &m0 = edge_idx(K)[0], &m1 = edge_idx(K)[1 + (L & ((1 << K) - 1))];
  const float *eb = p->pc_edge.as<float>();
  return {{eb + m0.u, eb + m1.u}, {eb + m0.v, eb + m1.v}, {m0.R, m1.R}, {m0.J, m1.J}, {m0.r, m1.r}};
}

// K3: both frame ends of a K-stage tile form added to its output, in one launch.
int add_frame_ends(zfft_plan *p, int K, const InDesc &in, const float2 *lo, float2 *out, int64_t nd,
                   int frames, hipStream_t st) {
  const EdgeMaps m = edge_maps(p, K, in.len);
  hipError_t e = launch_pc_edge(in, lo, out, nd, frames, m.U, m.V, m.R, m.J, m.r, st);
  if (e != hipSuccess) return hip_fail(e, "pc_edge launch");
  mark(p, st, "pc_edge");
  return ZFFT_OK;
}

// The PC runners: `frames` frames of in.len samples into p->pong (nd samples per frame), frame
// ends included.

// Zoom 2: the tail kernel straight on the mixed input.
int run_pc2_tiles(zfft_plan *p, const InDesc &in, int frames, int64_t nd, hipStream_t st) {
  hipError_t e = p->pong.ensure((size_t)frames * nd * sizeof(float2));
  if (e != hipSuccess) return fail(ZFFT_ENOMEM, "decimator workspace allocation failed");
  e = launch_pc2_tail(in, p->lo.as<float2>(), p->pong.as<float2>(), nd, frames, p->pc_tab2.as<PcTab2>(), st);
  if (e != hipSuccess) return hip_fail(e, "pc_tail launch");
  mark(p, st, "pc_tail");
  return add_frame_ends(p, 1, in, p->lo.as<float2>(), p->pong.as<float2>(), nd, frames, st);
}

// Zoom 4 as tiles: K1 (FIR alpha) -> y1 (ping) -> K2 -> out (pong).
int run_pc4_tiles(zfft_plan *p, const InDesc &in, int frames, int64_t nd, hipStream_t st) {
  const int64_t y1s = (pc4_y1_len(in.len) + kPc4K1M - 1) / kPc4K1M * kPc4K1M;
  hipError_t e = p->ping.ensure((size_t)frames * y1s * sizeof(float2));
  if (e == hipSuccess) e = p->pong.ensure((size_t)frames * nd * sizeof(float2));
  if (e != hipSuccess) return fail(ZFFT_ENOMEM, "decimator workspace allocation failed");
  e = launch_pc4_fir(in, p->lo.as<float2>(), p->ping.as<float2>(), y1s, frames, p->pc_tab4.as<PcTab4>(), st);
  if (e != hipSuccess) return hip_fail(e, "pc_fir launch");
  mark(p, st, "pc_fir");
  e = launch_pc4_tail(p->ping.as<float2>(), y1s, y1s, p->pong.as<float2>(), nd, frames,
                      p->pc_tab4.as<PcTab4>(), st);
  if (e != hipSuccess) return hip_fail(e, "pc_tail launch");
  mark(p, st, "pc_tail");
  return add_frame_ends(p, 2, in, p->lo.as<float2>(), p->pong.as<float2>(), nd, frames, st);
}

// Zoom 8 as tiles: K1 (FIRs) -> y2 (ping) -> K2 (own-rate sections, FIR, output-rate
// sections) -> out (pong) -> K3 (frame-end maps, in place).
int run_pc8_tiles(zfft_plan *p, const InDesc &in, int frames, int64_t nd, hipStream_t st) {
  const PcTab *tab = p->pc_tab.as<PcTab>();
  const int64_t y2s = (pc_y2_len(in.len) + kPcK1Q - 1) / kPcK1Q * kPcK1Q;
  hipError_t e = p->ping.ensure((size_t)frames * y2s * sizeof(float2));
  if (e == hipSuccess) e = p->pong.ensure((size_t)frames * nd * sizeof(float2));
  if (e != hipSuccess) return fail(ZFFT_ENOMEM, "decimator workspace allocation failed");
  e = launch_pc_fir(in, p->lo.as<float2>(), p->ping.as<float2>(), y2s, frames, tab, st);
  if (e != hipSuccess) return hip_fail(e, "pc_fir launch");
  mark(p, st, "pc_fir");
  e = launch_pc_tail(p->ping.as<float2>(), y2s, p->pong.as<float2>(), nd, frames, tab, st);
  if (e != hipSuccess) return hip_fail(e, "pc_tail launch");
  mark(p, st, "pc_tail");
  return add_frame_ends(p, kPcStages, in, p->lo.as<float2>(), p->pong.as<float2>(), nd, frames, st);
}

// One walk or FC launch over K stages, `in` with LO table `lo` into `out` (nd samples per
// frame), then the frame-end maps out += U (V^T x) behind it on the same stream.  fc_tab: the FC
// table (twiddles, then rows), or null for the walk (K = 2, 3).
int run_walk_into(zfft_plan *p, const InDesc &in, const float2 *lo, const float2 *fc_tab, int K, float2 *out,
                  int64_t nd, int frames, const char *name, hipStream_t st) {
  hipError_t e;
  if (fc_tab) e = launch_fc_decim(in, lo, fc_tab, kFcRow, out, nd, frames, 1 << K, st);
  else if (K == 2) e = launch_pc_walk4(in, lo, out, nd, frames, p->pc_tab4.as<PcTab4>(), st);
  else e = launch_pc_walk(in, lo, out, nd, frames, p->pc_tab.as<PcTab>(), st);
  if (e != hipSuccess) return hip_fail(e, fc_tab ? "fc_decim launch" : "pc_walk launch");
  mark(p, st, name);
  const EdgeMaps m = edge_maps(p, K, in.len);
  e = launch_pc_edge_batch(in, lo, out, nd, frames, m.U, m.V, m.R, m.J, m.r, st);
  if (e != hipSuccess) return hip_fail(e, "pc_edge launch");
  mark(p, st, "pc_edge");
  return ZFFT_OK;
}

// The walk (zoom 4 or 8: one launch, y2 -- zoom 4: y1 -- in LDS) or FC in its place
// (fc_kernels.hip; zoom 2 too) on the plan's input, into p->pong.
int run_walk(zfft_plan *p, const InDesc &in, int frames, int64_t nd, Head head, hipStream_t st) {
  const bool fc = head == Head::Fc2 || head == Head::Fc4 || head == Head::Fc8;
  const int K = head == Head::Fc2 ? 1 : head == Head::Fc4 || head == Head::Walk4 ? 2 : kPcStages;
  int rc;
  if (fc && (rc = ensure_fc(p, 1 << K))) return rc;
  hipError_t e = p->pong.ensure((size_t)frames * nd * sizeof(float2));
  if (e != hipSuccess) return fail(ZFFT_ENOMEM, "decimator workspace allocation failed");
  return run_walk_into(p, in, p->lo.as<float2>(), fc ? p->fc_tab.as<float2>() : nullptr, K,
                       p->pong.as<float2>(), nd, frames, fc ? "fc_decim" : K == 2 ? "pc_walk4" : "pc_walk", st);
}

// One PC / FC form over its stages: n[stages] samples per frame into p->pong.
int run_pc(zfft_plan *p, const InDesc &in, int frames, int64_t nd, Head head, hipStream_t st) {
  int rc = ensure_pc(p);
  if (rc) return rc;
  switch (head) {
    case Head::Pc2Tiles: return run_pc2_tiles(p, in, frames, nd, st);
    case Head::Pc4Tiles: return run_pc4_tiles(p, in, frames, nd, st);
    case Head::Pc8Tiles: return run_pc8_tiles(p, in, frames, nd, st);
    default: return run_walk(p, in, frames, nd, head, st);
  }
}

// Zoom >= 16: the PC / FC head (3 stages into pong), then stages 3 .. K-1 on its output (no LO
// mix): XA where XA takes the batch (ping, pong, ... in turn), else zoom 2's tiles and the
// exact blocked passes (few frames per call, the reference's one: a unit LO table stands for
// the mix their first pass applies).  Tail::Fc (path 7): FC launches first, three stages at a
// time and then the remaining two or one, each while its input has >= 16384 samples, on the
// unit LO table with the frame-end maps of its own zoom and input length.
int run_pc_head(zfft_plan *p, const InDesc &in, int frames, const std::vector<int64_t> &n,
                const Schedule &s, const float2 **out, hipStream_t st) {
  const int64_t n3 = n[kPcStages];
  hipError_t e = hipSuccess;
  if (s.tail != Tail::Xa) {  // ping / pong must not move under a stage's input once the tail sizes them
    const size_t G = (size_t)(frames + 63) / 64 * 64;
    // (after FC tail launches any later stage may be the blocked passes' first: both hold n3)
    const bool fct = s.tail == Tail::Fc;
    e = p->pong.ensure(std::max((size_t)frames * n3, fct ? G * n3 : p->K > kPcStages + 1 ? G * n[kPcStages + 2] : 0) *
                       sizeof(float2));
    if (e == hipSuccess) e = p->ping.ensure(G * (fct ? n3 : n[kPcStages + 1]) * sizeof(float2));
    if (e == hipSuccess && p->lo1_n < n3) {  // filled length, set only once the fill is enqueued
      e = p->lo1.ensure((size_t)n3 * sizeof(float2));
      if (e == hipSuccess) e = launch_fill_c64(p->lo1.as<float2>(), n3, 1.f, 0.f, st);
      if (e == hipSuccess) p->lo1_n = n3;
    }
    if (e != hipSuccess) return fail(ZFFT_ENOMEM, "decimator workspace allocation failed");
  }
  int rc = s.tail == Tail::Fc ? ensure_fc_tail(p) : ZFFT_OK;
  if (rc) return rc;
  rc = run_pc(p, in, frames, n3, s.head, st);
  if (rc) return rc;
  const float2 *cur = p->pong.as<float2>();
  if (s.tail != Tail::Xa) {
    int k = kPcStages;
    if (s.tail == Tail::Fc)
      for (int z; k < p->K && n[k] >= kPcMinL; k += z) {
        z = std::min(kPcStages, p->K - k);
        float2 *dst = cur == p->pong.as<float2>() ? p->ping.as<float2>() : p->pong.as<float2>();
        const InDesc src{cur, n[k], n[k], kInC64, 0};
        rc = run_walk_into(p, src, p->lo1.as<float2>(), p->fc_tail_tab.as<float2>() + fc_tail_off(1 << z), z, dst,
                           n[k + z], frames, "fc_tail", st);
        if (rc) return rc;
        cur = dst;
      }
    // zoom 2's tiles (XA's factorisation, the unit LO table) while a stage's input has >= 16384
    // samples, ping, pong, ... in turn; the blocked passes for the stages after that
    for (; k < p->K && n[k] >= kPcMinL; ++k) {
      float2 *dst = cur == p->pong.as<float2>() ? p->ping.as<float2>() : p->pong.as<float2>();
      const InDesc src{cur, n[k], n[k], kInC64, 0};
      e = launch_pc2_tail(src, p->lo1.as<float2>(), dst, n[k + 1], frames, p->pc_tab2.as<PcTab2>(), st);
      if (e != hipSuccess) return hip_fail(e, "pc_tail launch");
      mark(p, st, "pc_tail");
      rc = add_frame_ends(p, 1, src, p->lo1.as<float2>(), dst, n[k + 1], frames, st);
      if (rc) return rc;
      cur = dst;
    }
    if (k == p->K) {
      *out = cur;
      return ZFFT_OK;
    }
    const InDesc src{cur, n[k], n[k], kInC64, 0};
    return run_exact(p, src, p->lo1.as<float2>(), frames, n, out, st, 0, 0, k);
  }
  e = p->ping.ensure((size_t)frames * n[kPcStages + 1] * sizeof(float2));
  if (e != hipSuccess) return fail(ZFFT_ENOMEM, "decimator workspace allocation failed");
  for (int k = kPcStages; k < p->K; ++k) {
    float2 *dst = ((k - kPcStages) & 1) ? p->pong.as<float2>() : p->ping.as<float2>();
    const InDesc src{cur, n[k], n[k], kInC64, 0};
    e = launch_xa_stage(src, (int)n[k], p->lo.as<float2>(), false, dst, frames, p->xa_tab.as<XaTab>(), st);
    if (e != hipSuccess) return hip_fail(e, "xa_stage launch");
    mark(p, st, "xa_stage");
    cur = dst;
  }
  *out = cur;
  return ZFFT_OK;
}

}  // namespace

int run_decimator(zfft_plan *p, const InDesc &in, int64_t L, int frames,
                  const std::vector<int64_t> &n, const float2 **out, hipStream_t st) {
  const Schedule s = choose_schedule({p->K, (int)in_elem_bytes(p->cfg.in_dtype), p->path, L, frames});
  if (s.rc) return fail(s.rc, s.why);
  int rc = ensure_lo(p, L);
  if (rc) return rc;
  if (s.tail != Tail::None) return run_pc_head(p, in, frames, n, s, out, st);
  switch (s.head) {
    case Head::Exact: return run_exact(p, in, p->lo.as<float2>(), frames, n, out, st);
    case Head::Fused: return run_fused(p, in, L, frames, n, out, st);
    case Head::Xa: return run_xa(p, in, frames, n, out, st);
    default:
      rc = run_pc(p, in, frames, n[p->K], s.head, st);
      *out = p->pong.as<float2>();  // (sized by the runner)
      return rc;
  }
}

}  // namespace zfft
