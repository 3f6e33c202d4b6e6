// track_kernels.hip -- the emission tracker (zfft.h's rule of zfft_plan_track):
// connected components over the detector's runs of one pass, with the state carried from push
// to push on the device.  A node is a (row, slot) pair, numbered row-major: the frontier's
// G = gap + 1 rows first (local rows 0 .. G - 1, the last G rows given before this pass), then
// the pass's R rows (local rows G .. G + R - 1).
//
// The launches of a pass, each after the last on the one stream -- no workgroup ever waits for
// another, and every loop below has its bound in its head:
//   (memset)      the aggregates of every node to zero: every aggregate is kept in a form whose
//                 identity is 0 and whose merge is an integer max or add (a minimum as the
//                 maximum of the complement), so the atomics need no other initial value
//   track_label   one workgroup per chunk of rows: union-find in LDS over the links inside the
//                 chunk, parent[node] = the chunk's lowest node of the component, the runs'
//                 aggregates added to that node; one more workgroup seeds the frontier's nodes
//                 with the open table
//   track_seam    the links across a chunk's first row (into the chunk before, or the frontier):
//                 union-find in global memory, one thread per run of a chunk's first G rows
//   track_merge   parent[node] = the component's root; every chunk root's aggregates added to it
//   track_peak_row, track_peak_col   the tie-break of the peak: the lowest row, then the lowest
//                 column in that row, among the holders of the maximum (two more integer maxima,
//                 over the chunks' own peaks, which track_label settles in LDS)
//   track_count   per row the reported tracks that end in it (they all have a run there), and
//                 per workgroup of rows their sum
//   track_scan    exclusive prefix sum of the workgroups' sums; with the scan of a workgroup's
//                 rows in track_emit: the store positions
//   track_emit    the records into the store, in ascending (row_last, row_first, slot_first)
//   track_frontier  the counters; the last G rows and their components become the new frontier
//                 and open table
// Union-find: parent[x] <= x always, only a root is ever hooked (a compare-and-swap from x to a
// lower node), so a find is a strictly descending walk, the root of a component is its lowest
// node whatever the order of the unions, and a stale read only shows an ancestor.
// Columns are compared, never used as addresses; every index is derived from (row, slot).
#include <hip/hip_runtime.h>

#include "zfft_internal.h"

namespace zfft {

namespace {

constexpr int kT = kTrackThreads;

__device__ __forceinline__ uint32_t ord32(int32_t c) { return (uint32_t)c ^ 0x80000000u; }  // int order -> uint order
__device__ __forceinline__ int32_t unord32(uint32_t u) { return (int32_t)(u ^ 0x80000000u); }
// det_key (zfft_detect_keys.h) of peak_db with -0.0 taken as 0.0: the float comparison's order
__device__ __forceinline__ uint32_t peak_key(float v) {
  uint32_t u = __float_as_uint(v);
  if ((u & 0x7FFFFFFFu) == 0u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ int used_of(int32_t found, int K) { return min(max(found, 0), K); }
__device__ __forceinline__ int row_used(const TrackArgs &a, int lr) {
  return lr < a.G ? used_of(a.fr_found[lr], a.K) : used_of(a.found[lr - a.G], a.K);
}
__device__ __forceinline__ zfft_emission row_rec(const TrackArgs &a, int lr, int s) {
  return lr < a.G ? a.fr_ev[lr * a.K + s] : a.events[(int64_t)(lr - a.G) * a.K + s];
}
__device__ __forceinline__ int64_t global_row(const TrackArgs &a, int lr) { return a.t0 - a.G + lr; }
__device__ __forceinline__ bool linked(int fa, int la, int fb, int lb, int slack) {
  // in 64 bits: the device form promises nothing about the columns
  return (int64_t)fa <= (int64_t)lb + slack && (int64_t)fb <= (int64_t)la + slack;
}

// ---- union-find; SCOPE: workgroup for LDS, agent for global memory ----
// A walk reads through the caches (workgroup scope) in either memory: what it sees of another
// workgroup's hooks may be old, which is an ancestor all the same -- the compare-and-swap (SCOPE)
// is what decides, and a failed one returns the current parent.
template <int SCOPE>
__device__ __forceinline__ uint32_t uf_load(uint32_t *par, uint32_t x) {
  return __hip_atomic_load(par + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <int SCOPE, bool HALVE>
__device__ uint32_t uf_find(uint32_t *par, uint32_t x, uint32_t nodes) {
  for (uint32_t it = 0; it < nodes; ++it) {  // x falls every turn
    const uint32_t p = uf_load<SCOPE>(par, x);
    if (p == x) return x;
    if (HALVE) {
      const uint32_t g = uf_load<SCOPE>(par, p);
      if (g != p) __hip_atomic_fetch_min(par + x, g, __ATOMIC_RELAXED, SCOPE);  // x is no root: never hooked again
    }
    x = p;
  }
  return x;
}
template <int SCOPE, bool HALVE>
__device__ void uf_unite(uint32_t *par, uint32_t a, uint32_t b, uint32_t nodes) {
  for (uint32_t it = 0; it < 2u * nodes; ++it) {  // a + b falls every turn
    a = uf_find<SCOPE, HALVE>(par, a, nodes);
    b = uf_find<SCOPE, HALVE>(par, b, nodes);
    if (a == b) return;
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    uint32_t expect = a;  // hook the larger root under the smaller
    if (__hip_atomic_compare_exchange_strong(par + a, &expect, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE)) return;
    a = expect;  // someone hooked a first: expect < a
  }
}
// read-only walk to the root (between launches the forest does not change under a reader, but
// for track_merge's flattening stores, which only shorten a path)
__device__ __forceinline__ uint32_t uf_root(const uint32_t *par, uint32_t x, uint32_t nodes) {
  for (uint32_t it = 0; it < nodes; ++it) {
    const uint32_t p = par[x];
    if (p == x) return x;
    x = p;
  }
  return x;
}

using u64 = unsigned long long;

// the aggregates of run `e` in global row `row`, slot `s`, added to node `n`
__device__ __forceinline__ void add_run(const TrackArgs &a, uint32_t n, int64_t row, int s, const zfft_emission &e) {
  atomicMax((u64 *)a.a_name + n, ~(u64)((uint64_t)row * 32u + (uint32_t)s));
  atomicMax((u64 *)a.a_last + n, (u64)row + 1u);
  atomicAdd((u64 *)a.a_cells + n, (u64)((int64_t)e.last - (int64_t)e.first + 1));
  atomicAdd((u64 *)a.a_runs + n, (u64)1);
  atomicMax(a.a_colf + n, ~ord32(e.first));
  atomicMax(a.a_coll + n, ord32(e.last));
}

__device__ __forceinline__ TrackOpen load_agg(const TrackArgs &a, uint32_t n) {
  TrackOpen o;
  o.name = ~a.a_name[n];
  o.row_last = (int64_t)a.a_last[n] - 1;
  o.peak_row = (int64_t)~a.a_prow[n];
  o.cells = a.a_cells[n];
  o.runs = a.a_runs[n];
  o.col_first = unord32(~a.a_colf[n]);
  o.col_last = unord32(a.a_coll[n]);
  o.peak_col = unord32(~a.a_pcol[n]);  // (a_pcol holds ~ of the order-mapped column)
  o.peak_key = a.a_pkey[n];
  return o;
}

// ---- track_label ----
__global__ __launch_bounds__(kT) void track_label(TrackArgs a) {
  __shared__ int s_first[kTrackChunkNodes], s_last[kTrackChunkNodes];
  __shared__ uint32_t s_par[kTrackChunkNodes];
  __shared__ uint32_t s_key[kTrackChunkNodes];  // per chunk root: the maximum peak key of its runs
  __shared__ u64 s_pos[kTrackChunkNodes];       // and ~(row in the chunk, peak column) of its lowest holder
  __shared__ int s_used[64];
  __shared__ unsigned s_trunc;
  const int tid = threadIdx.x, K = a.K, G = a.G;
  if ((int)blockIdx.x == a.chunks) {  // the frontier's nodes: their representative, the open table
    for (int i = tid; i < G * K; i += kT) {
      const uint32_t rep = a.fr_parent[i];
      a.parent[i] = rep;
      if (rep == (uint32_t)i && i % K < used_of(a.fr_found[i / K], K)) {
        const TrackOpen o = a.open_tab[i];
        a.a_name[i] = ~o.name;
        a.a_last[i] = (uint64_t)o.row_last + 1u;
        a.a_cells[i] = o.cells;
        a.a_runs[i] = o.runs;
        a.a_colf[i] = ~ord32(o.col_first);
        a.a_coll[i] = ord32(o.col_last);
        a.a_pkey[i] = a.c_pkey[i] = o.peak_key;  // the track's peak so far: a candidate like a chunk's
        a.c_prow[i] = (uint64_t)o.peak_row;
        a.c_pcol[i] = ord32(o.peak_col);
      }
    }
    return;
  }
  const int r0 = (int)blockIdx.x * a.chunk_rows;          // first row of the chunk, in the pass
  const int rows = min(a.chunk_rows, a.R - r0);
  const int nC = rows * K;                                  // <= kTrackChunkNodes
  const uint32_t base = (uint32_t)(G + r0) * (uint32_t)K;  // node of the chunk's (row 0, slot 0)
  if (tid == 0) s_trunc = 0;
  __syncthreads();
  if (tid < rows) {
    const int32_t f = a.found[r0 + tid];
    s_used[tid] = used_of(f, K);
    if (f > K) atomicAdd(&s_trunc, 1u);
  }
  __syncthreads();
  for (int i = tid; i < nC; i += kT) {
    const int r = i / K, s = i - r * K;
    s_par[i] = (uint32_t)i;
    s_key[i] = 0;
    s_pos[i] = 0;
    if (s < s_used[r]) {
      const zfft_emission e = a.events[(int64_t)(r0 + r) * K + s];
      s_first[i] = e.first;
      s_last[i] = e.last;
    }
  }
  __syncthreads();
  if (tid == 0 && s_trunc) atomicAdd((u64 *)&a.ctr->truncated_rows, (u64)s_trunc);
  for (int i = tid; i < nC; i += kT) {  // the links inside the chunk
    const int r = i / K, s = i - r * K;
    if (s >= s_used[r]) continue;
    const int fb = s_first[i], lb = s_last[i];
    for (int dr = 1; dr <= G && dr <= r; ++dr) {
      const int ra = r - dr;
      for (int sa = 0; sa < s_used[ra]; ++sa) {
        const int j = ra * K + sa;
        if (linked(s_first[j], s_last[j], fb, lb, a.slack))
          uf_unite<__HIP_MEMORY_SCOPE_WORKGROUP, false>(s_par, (uint32_t)j, (uint32_t)i, (uint32_t)nC);
      }
    }
  }
  __syncthreads();
  constexpr int kPer = kTrackChunkNodes / kT;  // nodes of a thread
  uint32_t root[kPer], key[kPer];
  u64 pos[kPer];
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int i = tid + k * kT;
    key[k] = 0, pos[k] = 0, root[k] = 0;
    if (i >= nC) continue;
    const int r = i / K, s = i - r * K;
    root[k] = uf_find<__HIP_MEMORY_SCOPE_WORKGROUP, false>(s_par, (uint32_t)i, (uint32_t)nC);
    a.parent[base + i] = base + root[k];
    if (s >= s_used[r]) continue;
    const zfft_emission e = a.events[(int64_t)(r0 + r) * K + s];
    add_run(a, base + root[k], a.t0 + r0 + r, s, e);
    key[k] = peak_key(e.peak_db);
    pos[k] = ~(((u64)(uint32_t)r << 32) | ord32(e.peak));  // never 0: r < 64
    atomicMax(&s_key[root[k]], key[k]);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kPer; ++k)  // the holders of the chunk's maximum: the lowest (row, peak)
    if (pos[k] && s_key[root[k]] == key[k]) atomicMax(&s_pos[root[k]], pos[k]);
  __syncthreads();
  for (int i = tid; i < nC; i += kT) {  // a chunk root with runs: its candidate for the track's peak
    if (!s_pos[i]) continue;
    const u64 p = ~s_pos[i];
    a.a_pkey[base + i] = a.c_pkey[base + i] = s_key[i];
    a.c_prow[base + i] = (uint64_t)(a.t0 + r0) + (p >> 32);
    a.c_pcol[base + i] = (uint32_t)p;
  }
}

// ---- track_seam: thread = (chunk, row among the chunk's first G, slot) ----
__global__ __launch_bounds__(kT) void track_seam(TrackArgs a) {
  const int K = a.K, G = a.G;
  const int64_t gid = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (gid >= (int64_t)a.chunks * G * K) return;
  const int s = (int)(gid % K), j = (int)(gid / K % G), c = (int)(gid / K / G);
  const int r = c * a.chunk_rows + j;  // row in the pass
  if (j >= a.chunk_rows || r >= a.R) return;
  const int lr = G + r, lr0 = G + c * a.chunk_rows;  // local row; the chunk's first local row
  if (s >= row_used(a, lr)) return;
  const zfft_emission eb = row_rec(a, lr, s);
  const uint32_t nodes = (uint32_t)(a.R + G) * (uint32_t)K, nb = (uint32_t)lr * K + s;
  for (int dr = 1; dr <= G; ++dr) {
    const int la = lr - dr;  // >= 0: lr >= G
    if (la >= lr0) continue;  // inside the chunk: track_label's
    const int ua = row_used(a, la);
    for (int sa = 0; sa < ua; ++sa) {
      const zfft_emission ea = row_rec(a, la, sa);
      if (linked(ea.first, ea.last, eb.first, eb.last, a.slack))
        uf_unite<__HIP_MEMORY_SCOPE_AGENT, true>(a.parent, (uint32_t)la * K + sa, nb, nodes);
    }
  }
}

// ---- track_merge: thread = node ----
__global__ __launch_bounds__(kT) void track_merge(TrackArgs a) {
  const uint32_t nodes = (uint32_t)(a.R + a.G) * (uint32_t)a.K;
  const int64_t gid = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (gid >= nodes) return;
  const uint32_t n = (uint32_t)gid, root = uf_root(a.parent, n, nodes);
  if (root == n) return;
  a.parent[n] = root;
  const uint64_t runs = a.a_runs[n];  // a chunk's root (or a seeded frontier node) with something to give
  if (!runs) return;
  atomicMax((u64 *)a.a_name + root, (u64)a.a_name[n]);
  atomicMax((u64 *)a.a_last + root, (u64)a.a_last[n]);
  atomicAdd((u64 *)a.a_cells + root, (u64)a.a_cells[n]);
  atomicAdd((u64 *)a.a_runs + root, (u64)runs);
  atomicMax(a.a_colf + root, a.a_colf[n]);
  atomicMax(a.a_coll + root, a.a_coll[n]);
  atomicMax(a.a_pkey + root, a.a_pkey[n]);
}

// ---- track_peak_row / track_peak_col: thread = node; the candidates (the chunk roots with runs and
// the frontier's seeded nodes, each with the peak of its part) that hold the track's maximum ----
template <bool COL>
__global__ __launch_bounds__(kT) void track_peak(TrackArgs a) {
  const uint32_t nodes = (uint32_t)(a.R + a.G) * (uint32_t)a.K;
  const int64_t gid = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (gid >= nodes) return;
  const uint32_t n = (uint32_t)gid;
  if (!a.a_runs[n]) return;
  const uint32_t root = uf_root(a.parent, n, nodes);
  if (a.a_pkey[root] != a.c_pkey[n]) return;
  // (the plain reads of the running maximum may be old, that is lower: an atomic too many, never one too few)
  if (!COL) {
    const uint64_t v = ~a.c_prow[n];
    if (v > a.a_prow[root]) atomicMax((u64 *)a.a_prow + root, (u64)v);
  } else if (~a.a_prow[root] == a.c_prow[n]) {
    const uint32_t v = ~a.c_pcol[n];
    if (v > a.a_pcol[root]) atomicMax(a.a_pcol + root, v);
  }
}

// The track that ends in local row lr with its lowest run there in slot s: true, its record in
// *o and whether it is reported, when (lr, s) is that run.
__device__ __forceinline__ bool ends_here(const TrackArgs &a, int lr, int s, uint32_t nodes, uint32_t *root_out) {
  const uint32_t root = uf_root(a.parent, (uint32_t)lr * a.K + s, nodes);
  if ((int64_t)a.a_last[root] - 1 != global_row(a, lr)) return false;
  for (int s2 = 0; s2 < s; ++s2)
    if (uf_root(a.parent, (uint32_t)lr * a.K + s2, nodes) == root) return false;
  *root_out = root;
  return true;
}
__device__ __forceinline__ bool long_enough(const TrackArgs &a, uint32_t root) {
  const int64_t first = (int64_t)(~a.a_name[root] >> 5), last = (int64_t)a.a_last[root] - 1;
  return last - first + 1 >= (int64_t)a.min_rows;
}

// ---- track_count: thread = local row; the rows that close in this pass are lr < R ----
// rowcnt[lr] per row, and per workgroup (kT rows) their sum in rowoff[blockIdx.x]
__global__ __launch_bounds__(kT) void track_count(TrackArgs a) {
  __shared__ int s_tot;
  const int64_t gid = (int64_t)blockIdx.x * kT + threadIdx.x;
  const int lr = (int)gid;
  const uint32_t nodes = (uint32_t)(a.R + a.G) * (uint32_t)a.K;
  int cnt = 0, shorts = 0;
  if (threadIdx.x == 0) s_tot = 0;
  __syncthreads();
  if (gid < a.R) {
    const int u = row_used(a, lr);
    for (int s = 0; s < u; ++s) {
      uint32_t root;
      if (!ends_here(a, lr, s, nodes, &root)) continue;
      if (long_enough(a, root)) ++cnt;
      else ++shorts;
    }
  }
  if (gid < a.R + a.G) a.rowcnt[lr] = cnt;
  if (cnt) atomicAdd(&s_tot, cnt);
  if (shorts) atomicAdd((u64 *)&a.ctr->short_tracks, (u64)shorts);
  __syncthreads();
  if (threadIdx.x == 0) a.rowoff[blockIdx.x] = s_tot;
}

// ---- track_scan: one workgroup; rowoff[b] = exclusive prefix sum of track_count's workgroup
// sums (at most kTrackPassNodes / kT + 2 of them), the total to pending ----
__global__ __launch_bounds__(kTrackScanThreads) void track_scan(TrackArgs a) {
  __shared__ int s_sum[kTrackScanThreads];
  const int n = (a.R + a.G + kT - 1) / kT, tid = threadIdx.x;
  const int per = (n + kTrackScanThreads - 1) / kTrackScanThreads;
  const int lo = min(n, tid * per), hi = min(n, lo + per);
  int sum = 0;
  for (int i = lo; i < hi; ++i) sum += a.rowoff[i];
  s_sum[tid] = sum;
  __syncthreads();
  for (int d = 1; d < kTrackScanThreads; d *= 2) {  // inclusive scan of the threads' sums
    const int v = tid >= d ? s_sum[tid - d] : 0;
    __syncthreads();
    s_sum[tid] += v;
    __syncthreads();
  }
  int run = s_sum[tid] - sum;
  for (int i = lo; i < hi; ++i) {
    const int c = a.rowoff[i];
    a.rowoff[i] = run;
    run += c;
  }
  if (tid == kTrackScanThreads - 1) a.ctr->pending = (uint64_t)s_sum[tid];
}

// ---- track_emit: thread = local row, the workgroups as track_count's ----
__global__ __launch_bounds__(kT) void track_emit(TrackArgs a) {
  __shared__ int s_cnt[kT];
  const int64_t gid = (int64_t)blockIdx.x * kT + threadIdx.x;
  const int lr = (int)gid, tid = threadIdx.x;
  const int cnt = gid < a.R ? a.rowcnt[lr] : 0;
  s_cnt[tid] = cnt;
  __syncthreads();
  for (int d = 1; d < kT; d *= 2) {  // inclusive scan of the workgroup's rows
    const int v = tid >= d ? s_cnt[tid - d] : 0;
    __syncthreads();
    s_cnt[tid] += v;
    __syncthreads();
  }
  if (!cnt) return;
  const uint32_t nodes = (uint32_t)(a.R + a.G) * (uint32_t)a.K;
  const uint64_t base = a.ctr->unread + (uint64_t)a.rowoff[blockIdx.x] + (uint64_t)(s_cnt[tid] - cnt);
  const int u = row_used(a, lr);
  for (int s = 0; s < u; ++s) {
    uint32_t root;
    if (!ends_here(a, lr, s, nodes, &root) || !long_enough(a, root)) continue;
    const uint64_t name = ~a.a_name[root];
    int rank = 0;  // the row's reported tracks with a lower name
    for (int s2 = 0; s2 < u; ++s2) {
      uint32_t r2;
      if (s2 != s && ends_here(a, lr, s2, nodes, &r2) && long_enough(a, r2) && ~a.a_name[r2] < name) ++rank;
    }
    const uint64_t pos = base + (uint64_t)rank;
    if (pos < (uint64_t)a.max_tracks)
      a.store[(a.head + pos) % (uint64_t)a.max_tracks] = track_record(load_agg(a, root));
  }
}

// What thread 0 of the single-workgroup kernels does with `n` more reported tracks.
__device__ __forceinline__ void account(TrackCounters *c, uint64_t n, int max_tracks) {
  const uint64_t want = c->unread + n, keep = want < (uint64_t)max_tracks ? want : (uint64_t)max_tracks;
  c->dropped += want - keep;
  c->unread = keep;
  c->pending = 0;
}

// ---- track_frontier: one workgroup of kTrackFrontier threads, thread = new frontier node ----
__global__ __launch_bounds__(kTrackFrontier) void track_frontier(TrackArgs a) {
  __shared__ uint32_t s_root[kTrackFrontier];
  __shared__ int s_open;
  const int tid = threadIdx.x, K = a.K, G = a.G;
  const uint32_t nodes = (uint32_t)(a.R + G) * (uint32_t)K;
  const bool in = tid < G * K;
  const int j = in ? tid / K : 0, s = in ? tid - j * K : 0, lr = a.R + j;  // the last G local rows
  const int u = in ? row_used(a, lr) : 0;
  const bool act = in && s < u;
  zfft_emission e = {0, 0, 0, 0.f};
  uint32_t root = 0xFFFFFFFFu;
  if (act) {
    e = row_rec(a, lr, s);
    root = uf_root(a.parent, (uint32_t)lr * K + s, nodes);
  }
  s_root[tid] = root;
  if (tid == 0) {
    s_open = 0;
    account(a.ctr, a.ctr->pending, a.max_tracks);
  }
  __syncthreads();  // everything of the old frontier is read: it is overwritten from here on
  uint32_t rep = (uint32_t)tid;
  if (act)
    for (int i = 0; i < tid; ++i)
      if (s_root[i] == root) {
        rep = (uint32_t)i;
        break;
      }
  if (in) {
    a.fr_ev[tid] = e;
    a.fr_parent[tid] = rep;
    if (s == 0) a.fr_found[j] = u;
    if (act && rep == (uint32_t)tid) {
      a.open_tab[tid] = load_agg(a, root);
      atomicAdd(&s_open, 1);
    }
  }
  __syncthreads();
  if (tid == 0) a.ctr->open = (uint64_t)s_open;
}

// ---- track_flush: one workgroup; every open track closes as it stands ----
__global__ __launch_bounds__(kTrackFrontier) void track_flush(TrackArgs a) {
  __shared__ uint64_t s_last[kTrackFrontier], s_name[kTrackFrontier];
  __shared__ int s_rep, s_short;
  const int tid = threadIdx.x, K = a.K, G = a.G;
  const bool in = tid < G * K;
  const bool valid = in && a.fr_parent[tid] == (uint32_t)tid && tid % K < used_of(a.fr_found[tid / K], K);
  TrackOpen o = {};
  bool rep = false;
  if (valid) {
    o = a.open_tab[tid];
    rep = o.row_last - (int64_t)(o.name >> 5) + 1 >= (int64_t)a.min_rows;
  }
  s_last[tid] = rep ? (uint64_t)o.row_last : ~0ull;  // ~0: not reported (a row is below 2^58)
  s_name[tid] = o.name;
  if (tid == 0) s_rep = s_short = 0;
  const uint64_t unread = a.ctr->unread;
  __syncthreads();
  if (valid && !rep) atomicAdd(&s_short, 1);
  if (rep) {
    atomicAdd(&s_rep, 1);
    int rank = 0;
    for (int i = 0; i < kTrackFrontier; ++i)
      if (s_last[i] < s_last[tid] || (s_last[i] == s_last[tid] && s_name[i] < s_name[tid])) ++rank;
    const uint64_t pos = unread + (uint64_t)rank;
    if (pos < (uint64_t)a.max_tracks) a.store[(a.head + pos) % (uint64_t)a.max_tracks] = track_record(o);
  }
  if (in) {  // later rows link to nothing earlier
    a.fr_parent[tid] = (uint32_t)tid;
    if (tid % K == 0) a.fr_found[tid / K] = 0;
  }
  __syncthreads();
  if (tid == 0) {
    account(a.ctr, (uint64_t)s_rep, a.max_tracks);
    a.ctr->short_tracks += (uint64_t)s_short;
    a.ctr->open = 0;
  }
}

}  // namespace

const char *const kTrackStepNames[kTrackSteps] = {"track_label", "track_seam",  "track_merge", "track_peak_row",
                                                  "track_peak_col", "track_count", "track_scan",  "track_emit",
                                                  "track_frontier"};

hipError_t launch_track_step(int step, const TrackArgs &a, hipStream_t st) {
  if (a.K < 1 || a.K > kTrackMaxK || a.G < 1 || a.G > kTrackMaxGap + 1 || a.R < 1 || a.chunk_rows < 1 ||
      a.chunk_rows > 64 || a.chunk_rows * a.K > kTrackChunkNodes || a.chunks != (a.R + a.chunk_rows - 1) / a.chunk_rows ||
      (int64_t)(a.R + a.G) * a.K > kTrackPassNodes + kTrackFrontier || a.max_tracks < 1)
    return hipErrorInvalidValue;
  const int64_t nodes = (int64_t)(a.R + a.G) * a.K;
  auto blocks = [](int64_t n) { return dim3((unsigned)((n + kT - 1) / kT)); };
  switch (step) {
    case 0:
      hipLaunchKernelGGL(track_label, dim3(a.chunks + 1), dim3(kT), 0, st, a);
      break;
    case 1:
      hipLaunchKernelGGL(track_seam, blocks((int64_t)a.chunks * a.G * a.K), dim3(kT), 0, st, a);
      break;
    case 2:
      hipLaunchKernelGGL(track_merge, blocks(nodes), dim3(kT), 0, st, a);
      break;
    case 3:
      hipLaunchKernelGGL(track_peak<false>, blocks(nodes), dim3(kT), 0, st, a);
      break;
    case 4:
      hipLaunchKernelGGL(track_peak<true>, blocks(nodes), dim3(kT), 0, st, a);
      break;
    case 5:
      hipLaunchKernelGGL(track_count, blocks(a.R + a.G), dim3(kT), 0, st, a);
      break;
    case 6:
      hipLaunchKernelGGL(track_scan, dim3(1), dim3(kTrackScanThreads), 0, st, a);
      break;
    case 7:
      hipLaunchKernelGGL(track_emit, blocks(a.R), dim3(kT), 0, st, a);
      break;
    case 8:
      hipLaunchKernelGGL(track_frontier, dim3(1), dim3(kTrackFrontier), 0, st, a);
      break;
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_track_flush(const TrackArgs &a, hipStream_t st) {
  if (a.K < 1 || a.K > kTrackMaxK || a.G < 1 || a.G > kTrackMaxGap + 1 || a.max_tracks < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(track_flush, dim3(1), dim3(kTrackFrontier), 0, st, a);
  return hipGetLastError();
}

}  // namespace zfft
