// Note graph: the `graph` source of the score fusion (include/anorag.h, "Note graph").
//
//   graph   symmetric CSR on the device: rowptr int64 [n + 1], nbr int32 [2E], wt float64 [2E], neighbours ascending inside
//           a row.  Built by one stable device sort of the 2E directed edges keyed (row << 32 | neighbour); a key that
//           appears twice is a pair given twice.
//   PageRank (graph/graph_index.py:46, networkx _pagerank_scipy).  a[p] = (1 / S_i) * w_ij for entry p = (row j, neighbour
//           i) is formed once — a reciprocal times the weight, as scipy forms Q @ A — then every iteration is ONE pass over
//           the CSR: one thread per row j adds x[i] * a[p] in ascending i, starting from 0.0.  The two reductions of an
//           iteration (dangling mass, L1 change) are tree sums of one fixed shape (ng_tree below): no atomics, the same
//           bits on every run and on every grid size.
//   retrieve (graph/graph_retriever.py:61-92).  One SLOT per (query, valid seed): a [n] distance row (the bit pattern of a
//           non-negative double orders like the double, so the relaxation is a 64-bit integer atomicMin), a round stamp
//           that admits a node to the next frontier once per round, two frontiers and the list of touched nodes.  Rounds
//           run for all slots of a sub-batch at once until every frontier is empty; min is order-independent, so the
//           fixed point does not depend on the schedule.  The slots of a query are then merged in seed order through a
//           per-query owner row (integer atomicMin of the seed position), and the query's nodes are ordered by four stable
//           radix sorts (id, dist, seed position, score descending).  Slots and queries are reset from their touched /
//           result lists, never by an n-wide fill.
//   quality (graph/graph_quality.py:5-46).  Hop counts only: the weights are not read.  Components: every
//           node ends with the smallest node index of its component, by rounds of (hook: integer atomicMin of the smaller
//           label into the larger label's node, over the CSR entries; flatten: every node follows its labels to a root)
//           until a hook finds no edge between two labels.  Hop histogram: a pass walks 64 * W sources at once; a node has W
//           64-bit words in each of seen / frontier / next, bit j = source j of the pass, and a level is a pull over the
//           CSR (next[v] = OR of frontier[u] over the row & ~seen[v]) whose popcount is the number of (source, node) pairs
//           at that hop.  Only integers: the result does not depend on the schedule, the grid or W.
//
// This file is compiled with -ffp-contract=off (csrc/Makefile): `a * b + c` is two roundings, as in the reference.
#include <algorithm>
#include <cmath>
#include <limits>
#include <mutex>
#include <vector>

#include "common.hpp"

namespace anr {

typedef unsigned long long u64;

constexpr int kNgThreads = 256;
constexpr int kNgChunk = 1024;               // elements per workgroup of a tree sum: 4 per thread
constexpr u64 kNgInf = 0x7ff0000000000000ull;  // +inf: "not reached"
constexpr int kNgLanes = 16;                 // lanes that share one frontier node's row
constexpr int kNgMaxSlots = 32768;           // grid.y of the per-slot kernels

// ---- CSR build -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ng_edge_keys(const int64_t *src, const int64_t *dst, int64_t E, u64 *keys,
                                                      unsigned *vals) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= 2 * E) return;
  const int64_t e = p < E ? p : p - E;
  const u64 a = (u64)(p < E ? src[e] : dst[e]), b = (u64)(p < E ? dst[e] : src[e]);
  keys[p] = (a << 32) | b;
  vals[p] = (unsigned)p;
}

__global__ __launch_bounds__(256) void k_ng_csr_fill(const u64 *keys, const unsigned *vals, const double *w, int64_t E,
                                                     int32_t *nbr, double *wt, int *dup) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= 2 * E) return;
  nbr[p] = (int32_t)(keys[p] & 0xffffffffull);
  const int64_t v = vals[p];
  wt[p] = w[v < E ? v : v - E];
  if (p > 0 && keys[p] == keys[p - 1]) *dup = 1;
}

// rowptr[i] = the first sorted entry whose row is >= i
__global__ __launch_bounds__(256) void k_ng_rowptr(const u64 *keys, int64_t m, int64_t n, int64_t *rowptr) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  const u64 key = (u64)i << 32;
  int64_t lo = 0, hi = m;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  rowptr[i] = lo;
}

// ---- fixed-shape sums ------------------------------------------------------------------------------------------------
// ng_tree: the 256 values of a workgroup fold as v[t] += v[t + s] for s = 128, 64, ..., 1.  A chunk sum gives thread t the
// elements t, t + 256, t + 512, t + 768 of its 1024-element chunk, added in that order, then folds; the chunk sums are
// added the same way by one workgroup (thread t takes sums t, t + 256, ... in order, then the fold).  tests/notegraph_ref.py
// restates exactly this.
__device__ __forceinline__ double ng_tree(double v, double *sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int s = kNgThreads / 2; s > 0; s >>= 1) {
    if (t < s) sh[t] = sh[t] + sh[t + s];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void k_ng_rowsum(const int64_t *rowptr, const double *wt, int64_t n, double *inv) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) s = s + wt[e];
  inv[i] = s != 0.0 ? 1.0 / s : 0.0;  // 0.0 marks a dangling row (S == 0)
}

__global__ __launch_bounds__(256) void k_ng_scale(const int32_t *nbr, const double *wt, const double *inv, int64_t m,
                                                  double *a) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p < m) a[p] = inv[nbr[p]] * wt[p];
}

__global__ __launch_bounds__(256) void k_ng_fill_f64(double *x, int64_t n, double v) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] = v;
}

// chunk sums of the dangling rows' x
__global__ __launch_bounds__(256) void k_ng_dangling(const double *x, const double *inv, int64_t n, double *part) {
  __shared__ double sh[kNgThreads];
  double v = 0.0;
  for (int k = 0; k < kNgChunk / kNgThreads; ++k) {
    const int64_t i = (int64_t)blockIdx.x * kNgChunk + k * kNgThreads + threadIdx.x;
    if (i < n && inv[i] == 0.0) v = v + x[i];
  }
  v = ng_tree(v, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = v;
}

// workgroup b adds the chunk sums part[b][0 .. nb) into out[b]
__global__ __launch_bounds__(256) void k_ng_final(const double *part, int64_t nb, double *out) {
  __shared__ double sh[kNgThreads];
  const double *p = part + (int64_t)blockIdx.x * nb;
  double v = 0.0;
  for (int64_t i = threadIdx.x; i < nb; i += kNgThreads) v = v + p[i];
  v = ng_tree(v, sh);
  if (threadIdx.x == 0) out[blockIdx.x] = v;
}

struct NgStep {
  const int64_t *rowptr;
  const int32_t *nbr;
  const double *a, *x, *inv, *scal;  // scal[1] = the dangling mass of x
  double *xnew, *part;               // part[0][nb] L1 change, part[1][nb] dangling mass of xnew
  double alpha, p, omp;              // p = 1 / n, omp = (1 - alpha) * p
  int64_t n, nb;
};

__global__ __launch_bounds__(256) void k_ng_step(NgStep s) {
  __shared__ double sh[kNgThreads];
  const double dp = s.scal[1] * s.p;
  double err = 0.0, dang = 0.0;
  for (int k = 0; k < kNgChunk / kNgThreads; ++k) {
    const int64_t j = (int64_t)blockIdx.x * kNgChunk + k * kNgThreads + threadIdx.x;
    if (j >= s.n) continue;
    double acc = 0.0;
    for (int64_t e = s.rowptr[j]; e < s.rowptr[j + 1]; ++e) acc = acc + s.x[s.nbr[e]] * s.a[e];
    const double xn = s.alpha * (acc + dp) + s.omp;
    s.xnew[j] = xn;
    err = err + fabs(xn - s.x[j]);
    if (s.inv[j] == 0.0) dang = dang + xn;
  }
  err = ng_tree(err, sh);
  dang = ng_tree(dang, sh);
  if (threadIdx.x == 0) {
    s.part[blockIdx.x] = err;
    s.part[s.nb + blockIdx.x] = dang;
  }
}

// ---- retrieve --------------------------------------------------------------------------------------------------------
struct NgSlot {
  int32_t seed, pos, q;  // node, position in the query's seed list, query slot of the batch
};

struct NgSearch {
  const int64_t *rowptr;
  const int32_t *nbr;
  const double *wt;
  int64_t n;
  double cutoff;
  u64 *dist;        // [slots][n]
  int *stamp;       // [slots][n] last round that put the node into a frontier
  int *touched;     // [slots][n] nodes reached (without the seed), in arrival order
  int *fin, *fout;  // [slots][n]
  int *cnt_in, *cnt_out, *tcnt;  // [slots]
  const NgSlot *slot;
  int nslots, round;
  // merge
  int *owner;       // [qslots][n] lowest seed position that reached the node
  int *res_id, *res_pos;
  double *res_dist;  // [qslots][n]
  int *rcnt;         // [qslots]
};

__global__ __launch_bounds__(256) void k_ng_seed(NgSearch p) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= p.nslots) return;
  const int64_t base = (int64_t)s * p.n;
  p.dist[base + p.slot[s].seed] = 0ull;
  p.fin[base] = p.slot[s].seed;
  p.cnt_in[s] = 1;
  p.cnt_out[s] = 0;
  p.tcnt[s] = 0;
}

// one round: every frontier node u relaxes its row, kNgLanes lanes to a node
__global__ __launch_bounds__(256) void k_ng_relax(NgSearch p) {
  const int s = blockIdx.y;
  const int64_t g = ((int64_t)blockIdx.x * 256 + threadIdx.x) / kNgLanes;
  const int lane = threadIdx.x % kNgLanes;
  if (g >= p.cnt_in[s]) return;
  const int64_t base = (int64_t)s * p.n;
  const int u = p.fin[base + g];
  const double du = __longlong_as_double((long long)p.dist[base + u]);
  for (int64_t e = p.rowptr[u] + lane; e < p.rowptr[u + 1]; e += kNgLanes) {
    const double cand = du + p.wt[e];
    if (!(cand <= p.cutoff)) continue;
    const int v = p.nbr[e];
    const u64 cb = (u64)__double_as_longlong(cand);
    const u64 old = atomicMin(&p.dist[base + v], cb);
    if (cb < old) {
      if (old == kNgInf) p.touched[base + atomicAdd(&p.tcnt[s], 1)] = v;           // once per node: <= n - 1 entries
      if (atomicMax(&p.stamp[base + v], p.round) < p.round)                          // once per node and round: <= n
        p.fout[base + atomicAdd(&p.cnt_out[s], 1)] = v;
    }
  }
}

__global__ __launch_bounds__(256) void k_ng_owner(NgSearch p) {
  const int s = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.tcnt[s]) return;
  const int v = p.touched[(int64_t)s * p.n + i];
  atomicMin(&p.owner[(int64_t)p.slot[s].q * p.n + v], p.slot[s].pos);
}

__global__ __launch_bounds__(256) void k_ng_emit(NgSearch p) {
  const int s = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.tcnt[s]) return;
  const int64_t base = (int64_t)s * p.n, qb = (int64_t)p.slot[s].q * p.n;
  const int v = p.touched[base + i];
  if (p.owner[qb + v] != p.slot[s].pos) return;
  const int j = atomicAdd(&p.rcnt[p.slot[s].q], 1);  // a node has one owner: <= n entries per query
  p.res_id[qb + j] = v;
  p.res_pos[qb + j] = p.slot[s].pos;
  p.res_dist[qb + j] = __longlong_as_double((long long)p.dist[base + v]);
}

// the slot back to "nothing reached", from its touched list
__global__ __launch_bounds__(256) void k_ng_reset(NgSearch p) {
  const int s = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t base = (int64_t)s * p.n;
  if (i == 0) p.dist[base + p.slot[s].seed] = kNgInf;
  if (i >= p.tcnt[s]) return;
  const int v = p.touched[base + i];
  p.dist[base + v] = kNgInf;
  p.stamp[base + v] = 0;
}

__global__ __launch_bounds__(256) void k_ng_fill_u64(u64 *x, int64_t n, u64 v) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] = v;
}
__global__ __launch_bounds__(256) void k_ng_fill_i32(int *x, int64_t n, int v) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] = v;
}

struct NgOrder {
  const int *res_id, *res_pos;
  const double *res_dist, *cent, *imp;
  double *score;
  int *owner;  // the query's owner row
  int64_t f;
};

// graph_score of the query's f nodes (graph_retriever.py:87), the first sort key (id) and the owner row's reset
__global__ __launch_bounds__(256) void k_ng_score(NgOrder o, u64 *keys, unsigned *vals) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= o.f) return;
  const int id = o.res_id[j];
  o.score[j] = (o.cent[id] / (o.res_dist[j] + 1e-5)) * o.imp[id];
  keys[j] = (u64)id;
  vals[j] = (unsigned)j;
  o.owner[id] = 0x7fffffff;
}

// keys[i] of the next stable pass, read through the permutation so far: 0 dist, 1 seed position, 2 score (ascending
// image of the double; the pass sorts it descending), 3 id
__global__ __launch_bounds__(256) void k_ng_keys(NgOrder o, const unsigned *perm, int64_t m, int what, u64 *keys) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const unsigned j = perm[i];
  u64 k;
  if (what == 0) {
    k = (u64)__double_as_longlong(o.res_dist[j]);
  } else if (what == 1) {
    k = (u64)o.res_pos[j];
  } else if (what == 2) {
    const u64 b = (u64)__double_as_longlong(o.score[j]);
    k = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
  } else {
    k = (u64)o.res_id[j];
  }
  keys[i] = k;
}

__global__ __launch_bounds__(256) void k_ng_out_host(NgOrder o, const unsigned *perm, int64_t m, int64_t cap, int64_t *ids,
                                                     double *dist, double *score, int32_t *pos) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= cap) return;
  const bool live = i < m;
  const unsigned j = live ? perm[i] : 0u;
  ids[i] = live ? (int64_t)o.res_id[j] : -1;
  dist[i] = live ? o.res_dist[j] : __longlong_as_double(0x7ff8000000000000ll);
  score[i] = live ? o.score[j] : __longlong_as_double(0x7ff8000000000000ll);
  pos[i] = live ? o.res_pos[j] : -1;
}

__global__ __launch_bounds__(256) void k_ng_out_dev(NgOrder o, const unsigned *perm, int64_t m, int64_t cap, uint32_t *ids,
                                                    double *score, int32_t *count) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i == 0) *count = (int32_t)m;
  if (i >= cap) return;
  const bool live = i < m;
  const unsigned j = live ? perm[i] : 0u;
  ids[i] = live ? (uint32_t)o.res_id[j] : 0u;
  score[i] = live ? o.score[j] : 0.0;
}

__global__ __launch_bounds__(256) void k_ng_scatter_rows(const uint32_t *ids, const double *scores, const int32_t *count,
                                                         int64_t cap, int64_t n, double *out) {
  const int64_t q = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count[q] || i >= cap) return;
  const uint32_t id = ids[q * cap + i];
  if (id < n) out[q * n + id] = scores[q * cap + i];
}

// ---- graph quality: components ---------------------------------------------------------------------------------------
constexpr int kNgBfsWords = 16;  // default words per node and pass: a node's row of words is one 128-byte line (§5i)

__global__ __launch_bounds__(256) void k_ng_iota_i32(int32_t *x, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] = (int32_t)i;
}

// Every label is a node of the same component with label[x] <= x, before and after.  An edge between two labels lowers
// the larger label's node to the smaller label; each undirected edge is looked at from its larger end.
__global__ __launch_bounds__(256) void k_ng_cc_hook(const int64_t *rowptr, const int32_t *nbr, int64_t n, int32_t *label,
                                                    int *changed) {
  const int64_t u = ((int64_t)blockIdx.x * 256 + threadIdx.x) / kNgLanes;
  const int lane = threadIdx.x % kNgLanes;
  if (u >= n) return;
  const int32_t lu = __atomic_load_n(&label[u], __ATOMIC_RELAXED);
  bool any = false;
  for (int64_t e = rowptr[u] + lane; e < rowptr[u + 1]; e += kNgLanes) {
    const int32_t v = nbr[e];
    if (v >= u) continue;
    const int32_t lv = __atomic_load_n(&label[v], __ATOMIC_RELAXED);
    if (lu == lv) continue;
    atomicMin(&label[lu > lv ? lu : lv], lu > lv ? lv : lu);
    any = true;
  }
  if (any) *changed = 1;
}

// label[v] = the root its labels lead to.  Labels only fall and only thread v stores label[v], so a walk that meets
// another thread's store still ends at a root of v's component.
__global__ __launch_bounds__(256) void k_ng_cc_flatten(int32_t *label, int64_t n) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  int32_t l = __atomic_load_n(&label[v], __ATOMIC_RELAXED);
  for (;;) {
    const int32_t ll = __atomic_load_n(&label[l], __ATOMIC_RELAXED);
    if (ll == l) break;
    l = ll;
  }
  __atomic_store_n(&label[v], l, __ATOMIC_RELAXED);
}

// the sum of a workgroup's per-thread counts, valid in thread 0
__device__ __forceinline__ unsigned ng_count_block(unsigned c, unsigned *sh) {
  for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}

__global__ __launch_bounds__(256) void k_ng_cc_roots(const int32_t *label, int64_t n, u64 *count) {
  __shared__ unsigned sh[kNgThreads / 64];
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const unsigned c = ng_count_block(v < n && label[v] == (int32_t)v ? 1u : 0u, sh);
  if (threadIdx.x == 0 && c) atomicAdd(count, (u64)c);
}

// ---- graph quality: hop histogram ------------------------------------------------------------------------------------
struct NgBfs {
  const int64_t *rowptr;
  const int32_t *nbr;
  const int32_t *src;  // the pass's sources, or NULL: source j is node base + j
  int64_t n, base, nbits;  // nbits: sources of this pass, <= 64 * W
  int W, wshift;       // words per node, log2
  const u64 *fin;      // [n][W] frontier
  u64 *fout, *seen;    // [n][W]
  u64 *cnt;            // [2] pair counts of this level (slot) and of the next (zeroed here)
  int slot;
};

// seen = frontier = the sources' own bits (both zero before).  Two sources of one word that are the same node store the
// same word: each ORs in the bits of every source of its word that names its node.
__global__ __launch_bounds__(256) void k_ng_bfs_seed(NgBfs p, u64 *fin) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= p.nbits) return;
  const int64_t s = p.src ? (int64_t)p.src[j] : p.base + j;
  u64 bits = 1ull << (j & 63);
  if (p.src) {
    const int64_t g0 = j & ~63ll, g1 = g0 + 64 < p.nbits ? g0 + 64 : p.nbits;
    for (int64_t k = g0; k < g1; ++k)
      if (p.src[k] == (int32_t)s) bits |= 1ull << (k - g0);
  }
  const int64_t i = s * p.W + (j >> 6);
  p.seen[i] = bits;
  fin[i] = bits;
}

// One level, pull form.  Lane w of a node's W adjacent lanes owns word w: a neighbour's row of words is one contiguous
// load of the group.  A word whose pass bits are all seen can gain nothing and skips its row.
__global__ __launch_bounds__(256) void k_ng_bfs_level(NgBfs p) {
  __shared__ unsigned sh[kNgThreads / 64];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // = v * W + w
  const int64_t v = i >> p.wshift;
  const int w = (int)(i & (p.W - 1));
  unsigned c = 0;
  if (v < p.n) {
    const int64_t lo = (int64_t)w * 64;
    const u64 full = p.nbits >= lo + 64 ? ~0ull : p.nbits > lo ? (1ull << (p.nbits - lo)) - 1 : 0ull;
    const u64 s = p.seen[i];
    u64 nx = 0;
    if (~s & full) {
      u64 a0 = 0, a1 = 0, a2 = 0, a3 = 0;
      int64_t e = p.rowptr[v];
      const int64_t end = p.rowptr[v + 1];
      for (; e + 4 <= end; e += 4) {
        const int64_t u0 = p.nbr[e], u1 = p.nbr[e + 1], u2 = p.nbr[e + 2], u3 = p.nbr[e + 3];
        a0 |= p.fin[(u0 << p.wshift) + w];
        a1 |= p.fin[(u1 << p.wshift) + w];
        a2 |= p.fin[(u2 << p.wshift) + w];
        a3 |= p.fin[(u3 << p.wshift) + w];
      }
      for (; e < end; ++e) a0 |= p.fin[((int64_t)p.nbr[e] << p.wshift) + w];
      nx = (a0 | a1 | a2 | a3) & ~s;
      if (nx) p.seen[i] = s | nx;
    }
    p.fout[i] = nx;
    c = (unsigned)__popcll(nx);
  }
  c = ng_count_block(c, sh);
  if (threadIdx.x == 0) {
    if (c) atomicAdd(&p.cnt[p.slot], (u64)c);
    if (blockIdx.x == 0) p.cnt[p.slot ^ 1] = 0ull;  // the next level's counter: no launch in flight uses it
  }
}

}  // namespace anr

using namespace anr;

struct anr_notegraph {
  int device = 0;
  int64_t n = 0, E = 0, m = 0;  // m = 2E CSR entries
  DevBuf<int64_t> rowptr;
  DevBuf<int32_t> nbr;
  DevBuf<double> wt, cent, imp;
  hipStream_t stream = nullptr;
  std::mutex mu;
  int64_t max_slots = 0;
  // retrieve workspace, kept between calls; between calls every dist is +inf, every stamp 0, every owner INT_MAX
  int ws_slots = 0, ws_q = 0;
  bool ws_slots_limited = false, ws_q_limited = false;  // sized by free memory, not by the call that asked
  int64_t ws_cap = 0;
  struct Workspace {
    DevBuf<u64> dist;
    DevBuf<int> stamp, touched, fa, fb, cnt_a, cnt_b, tcnt;
    DevBuf<NgSlot> slot;
    DevBuf<int> owner, res_id, res_pos, rcnt;
    DevBuf<double> res_dist;
    DevBuf<u64> key_a, key_b;
    DevBuf<unsigned> val_a, val_b;
    DevBuf<double> score;
    DevBuf<unsigned char> sort_temp;
    DevBuf<int64_t> o_ids;  // [ws_q][ws_cap] staging of the host outputs
    DevBuf<double> o_dist, o_score;
    DevBuf<int32_t> o_pos;
  } ws;
  // graph quality workspace (components, hop histogram): its own buffers, grown when a call needs more, freed at destroy;
  // it shares nothing with the retrieve workspace above
  int64_t bfs_words = 0;      // ANR_NOTEGRAPH_OPT_BFS_WORDS, 0 = kNgBfsWords
  DevBuf<u64> q_state;        // seen, frontier, next: 3 x [n][W]
  DevBuf<int32_t> q_src;      // the explicit sources of a call
  DevBuf<int32_t> q_label;    // [n]
  DevBuf<u64> q_cnt;          // [2] level counters, [2] root count
  DevBuf<int> q_flag;
};

namespace {

inline unsigned blocks(int64_t n, int per = 256) { return (unsigned)std::max<int64_t>(1, ceil_div(n, per)); }

void free_workspace(anr_notegraph *h) {
  h->ws = anr_notegraph::Workspace{};
  h->ws_slots = h->ws_q = 0;
  h->ws_cap = 0;
  h->ws_slots_limited = h->ws_q_limited = false;
}

int ensure_quality_small(anr_notegraph *h) {
  ANR_TRY(h->q_cnt.alloc(4, "note graph"));
  ANR_TRY(h->q_flag.alloc(1, "note graph"));
  return ANR_OK;
}

// bytes per (query, seed) slot, per query of a batch, and shared by all
int64_t slot_bytes(int64_t n) { return 24 * n + 64; }
int64_t query_bytes(int64_t n, int64_t cap) { return 20 * n + 28 * cap + 64; }
int64_t shared_bytes(int64_t n) { return 32 * n + (int64_t)radix_sort_temp_bytes(n); }

// Sizes the workspace for a call: `want_slots` searches and `want_q` queries would run it in one sub-batch.
int ensure_workspace(anr_notegraph *h, int64_t want_slots, int64_t want_q, int64_t cap, bool host_out) {
  const int64_t n = h->n;
  want_slots = std::max<int64_t>(1, std::min<int64_t>(want_slots, kNgMaxSlots));
  want_q = std::max<int64_t>(1, want_q);
  if (h->max_slots > 0) {
    want_slots = std::min(want_slots, h->max_slots);
    want_q = std::min(want_q, h->max_slots);
  }
  const int64_t ocap = host_out ? cap : 0;
  if (h->ws.dist.p && (h->ws_slots >= want_slots || h->ws_slots_limited) && (h->ws_q >= want_q || h->ws_q_limited) &&
      h->ws_cap >= ocap)
    return ANR_OK;
  // the held workspace is too small (or of another shape): sized anew from the memory that is free without it
  free_workspace(h);
  size_t free_b = 0, total_b = 0;
  ANR_HIP(hipMemGetInfo(&free_b, &total_b));
  const int64_t budget = (int64_t)(free_b / 2) - shared_bytes(n);
  if (budget < query_bytes(n, ocap) + slot_bytes(n))
    return fail(ANR_EHIP, "note graph: %lld bytes of free device memory do not hold one search slot of %lld nodes",
                (long long)free_b, (long long)n);
  // a quarter of the budget to the queries of a batch (owner row, result list, output staging), the rest to the slots
  const int64_t nq_b = std::min(want_q, std::max<int64_t>(1, budget / 4 / query_bytes(n, ocap)));
  const int64_t ns_b = std::min(want_slots, std::max<int64_t>(1, (budget - nq_b * query_bytes(n, ocap)) / slot_bytes(n)));
  h->ws_q_limited = nq_b < want_q && !(h->max_slots > 0 && nq_b == h->max_slots);
  h->ws_slots_limited = ns_b < want_slots;
  ANR_TRY(h->ws.dist.alloc(ns_b * n, "note graph"));
  ANR_TRY(h->ws.stamp.alloc(ns_b * n, "note graph"));
  ANR_TRY(h->ws.touched.alloc(ns_b * n, "note graph"));
  ANR_TRY(h->ws.fa.alloc(ns_b * n, "note graph"));
  ANR_TRY(h->ws.fb.alloc(ns_b * n, "note graph"));
  ANR_TRY(h->ws.cnt_a.alloc(ns_b, "note graph"));
  ANR_TRY(h->ws.cnt_b.alloc(ns_b, "note graph"));
  ANR_TRY(h->ws.tcnt.alloc(ns_b, "note graph"));
  ANR_TRY(h->ws.slot.alloc(ns_b, "note graph"));
  ANR_TRY(h->ws.owner.alloc(nq_b * n, "note graph"));
  ANR_TRY(h->ws.res_id.alloc(nq_b * n, "note graph"));
  ANR_TRY(h->ws.res_pos.alloc(nq_b * n, "note graph"));
  ANR_TRY(h->ws.res_dist.alloc(nq_b * n, "note graph"));
  ANR_TRY(h->ws.rcnt.alloc(nq_b, "note graph"));
  ANR_TRY(h->ws.key_a.alloc(n, "note graph"));
  ANR_TRY(h->ws.key_b.alloc(n, "note graph"));
  ANR_TRY(h->ws.val_a.alloc(n, "note graph"));
  ANR_TRY(h->ws.val_b.alloc(n, "note graph"));
  ANR_TRY(h->ws.score.alloc(n, "note graph"));
  ANR_TRY(h->ws.sort_temp.alloc((int64_t)radix_sort_temp_bytes(n), "note graph"));
  if (ocap > 0) {
    ANR_TRY(h->ws.o_ids.alloc(nq_b * ocap, "note graph"));
    ANR_TRY(h->ws.o_dist.alloc(nq_b * ocap, "note graph"));
    ANR_TRY(h->ws.o_score.alloc(nq_b * ocap, "note graph"));
    ANR_TRY(h->ws.o_pos.alloc(nq_b * ocap, "note graph"));
  }
  // the one n-wide fill of a slot's life: when it is allocated
  hipLaunchKernelGGL(k_ng_fill_u64, dim3(blocks(ns_b * n)), dim3(256), 0, h->stream, h->ws.dist.p, ns_b * n, kNgInf);
  hipLaunchKernelGGL(k_ng_fill_i32, dim3(blocks(ns_b * n)), dim3(256), 0, h->stream, h->ws.stamp.p, ns_b * n, 0);
  hipLaunchKernelGGL(k_ng_fill_i32, dim3(blocks(nq_b * n)), dim3(256), 0, h->stream, h->ws.owner.p, nq_b * n, 0x7fffffff);
  ANR_HIP(hipGetLastError());
  h->ws_slots = (int)ns_b;
  h->ws_q = (int)nq_b;
  h->ws_cap = ocap;
  return ANR_OK;
}

// the searches of `ns` slots (already in h->ws.slot) to their fixed point, merged into their queries' result lists
int run_slots(anr_notegraph *h, const std::vector<NgSlot> &slots, int64_t s0, int ns, double cutoff) {
  hipStream_t st = h->stream;
  const anr_notegraph::Workspace &ws = h->ws;
  ANR_HIP(hipMemcpyAsync(ws.slot.p, slots.data() + s0, (size_t)ns * sizeof(NgSlot), hipMemcpyHostToDevice, st));
  NgSearch p{};
  p.rowptr = h->rowptr.p; p.nbr = h->nbr.p; p.wt = h->wt.p; p.n = h->n; p.cutoff = cutoff;
  p.dist = ws.dist.p; p.stamp = ws.stamp.p; p.touched = ws.touched.p;
  p.fin = ws.fa.p; p.fout = ws.fb.p; p.cnt_in = ws.cnt_a.p; p.cnt_out = ws.cnt_b.p; p.tcnt = ws.tcnt.p;
  p.slot = ws.slot.p; p.nslots = ns; p.round = 0;
  p.owner = ws.owner.p; p.res_id = ws.res_id.p; p.res_pos = ws.res_pos.p; p.res_dist = ws.res_dist.p; p.rcnt = ws.rcnt.p;
  hipLaunchKernelGGL(k_ng_seed, dim3(blocks(ns)), dim3(256), 0, st, p);
  std::vector<int> cnt((size_t)ns);
  int64_t maxc = 1;
  while (maxc > 0) {
    p.round += 1;
    hipLaunchKernelGGL(k_ng_relax, dim3(blocks(maxc * kNgLanes), (unsigned)ns), dim3(256), 0, st, p);
    ANR_HIP(hipMemcpyAsync(cnt.data(), p.cnt_out, (size_t)ns * sizeof(int), hipMemcpyDeviceToHost, st));
    ANR_HIP(hipMemsetAsync(p.cnt_in, 0, (size_t)ns * sizeof(int), st));  // the next round's output counter
    ANR_HIP(hipStreamSynchronize(st));
    maxc = 0;
    for (int c : cnt) maxc = std::max<int64_t>(maxc, c);
    std::swap(p.fin, p.fout);
    std::swap(p.cnt_in, p.cnt_out);
  }
  ANR_HIP(hipMemcpyAsync(cnt.data(), p.tcnt, (size_t)ns * sizeof(int), hipMemcpyDeviceToHost, st));
  ANR_HIP(hipStreamSynchronize(st));
  int64_t maxt = 0;
  for (int c : cnt) maxt = std::max<int64_t>(maxt, c);
  const dim3 grid(blocks(maxt), (unsigned)ns);
  hipLaunchKernelGGL(k_ng_owner, grid, dim3(256), 0, st, p);
  hipLaunchKernelGGL(k_ng_emit, grid, dim3(256), 0, st, p);
  hipLaunchKernelGGL(k_ng_reset, grid, dim3(256), 0, st, p);
  ANR_HIP(hipGetLastError());
  return ANR_OK;
}

int check_seeds(const anr_notegraph *h, int64_t nq, const int64_t *seed_offs, const int64_t *seeds, double cutoff,
                int64_t cap) {
  if (!h || nq < 0 || !seed_offs) return fail(ANR_EINVAL, "bad argument");
  if (seed_offs[0] != 0) return fail(ANR_EINVAL, "seed_offs[0] must be 0");
  for (int64_t q = 0; q < nq; ++q) {
    if (seed_offs[q + 1] < seed_offs[q]) return fail(ANR_EINVAL, "seed_offs must be non-decreasing");
    if (seed_offs[q + 1] - seed_offs[q] > 0x7fffffffll) return fail(ANR_EINVAL, "too many seeds in one query");
  }
  if (seed_offs[nq] > 0 && !seeds) return fail(ANR_EINVAL, "null seeds");
  if (!(cutoff >= 0.0)) return fail(ANR_EINVAL, "cutoff must be a non-negative number");
  if (cap < 1) return fail(ANR_EINVAL, "cap must be >= 1");
  return ANR_OK;
}

// Both retrieve entry points.  Host form: out_* host arrays; device form: ids_dev / scores_dev / count_dev.
int retrieve_impl(anr_notegraph *h, int64_t nq, const int64_t *seed_offs, const int64_t *seeds, double cutoff,
                  int64_t cap, bool host_out, int64_t *out_ids, double *out_dist, double *out_score, int32_t *out_pos,
                  int32_t *out_count, uint32_t *ids_dev, double *scores_dev, int32_t *count_dev) {
  if (nq == 0) return ANR_OK;
  const int64_t n = h->n;
  hipStream_t st = h->stream;
  const anr_notegraph::Workspace &ws = h->ws;  // sized below; the buffers themselves do not move
  // the busiest batch this call could form: every query, every valid seed
  int64_t valid = 0;
  for (int64_t e = 0; e < seed_offs[nq]; ++e) valid += (seeds[e] >= 0 && seeds[e] < n);
  ANR_TRY(ensure_workspace(h, valid, nq, cap, host_out));
  std::vector<NgSlot> slots;
  std::vector<int> found;
  for (int64_t q0 = 0; q0 < nq; q0 += h->ws_q) {
    const int nqb = (int)std::min<int64_t>(h->ws_q, nq - q0);
    slots.clear();
    for (int ql = 0; ql < nqb; ++ql)
      for (int64_t e = seed_offs[q0 + ql]; e < seed_offs[q0 + ql + 1]; ++e)
        if (seeds[e] >= 0 && seeds[e] < n)
          slots.push_back(NgSlot{(int32_t)seeds[e], (int32_t)(e - seed_offs[q0 + ql]), ql});
    ANR_HIP(hipMemsetAsync(ws.rcnt.p, 0, (size_t)nqb * sizeof(int), st));
    // slots in (query, seed position) order: an earlier sub-batch holds the earlier seeds of a query, so the owner row
    // it leaves behind already belongs to them
    for (int64_t s0 = 0; s0 < (int64_t)slots.size(); s0 += h->ws_slots)
      ANR_TRY(run_slots(h, slots, s0, (int)std::min<int64_t>(h->ws_slots, (int64_t)slots.size() - s0), cutoff));
    found.assign((size_t)nqb, 0);
    ANR_HIP(hipMemcpyAsync(found.data(), ws.rcnt.p, (size_t)nqb * sizeof(int), hipMemcpyDeviceToHost, st));
    ANR_HIP(hipStreamSynchronize(st));
    for (int ql = 0; ql < nqb; ++ql) {
      const int64_t f = found[ql], m = std::min<int64_t>(f, cap), q = q0 + ql;
      NgOrder o{};
      o.res_id = ws.res_id.p + (int64_t)ql * n; o.res_pos = ws.res_pos.p + (int64_t)ql * n;
      o.res_dist = ws.res_dist.p + (int64_t)ql * n; o.cent = h->cent.p; o.imp = h->imp.p; o.score = ws.score.p;
      o.owner = ws.owner.p + (int64_t)ql * n; o.f = f;
      const unsigned *perm = ws.val_a.p;
      if (f > 0) {
        // four stable passes, least significant key first: id, dist, seed position, score (descending)
        hipLaunchKernelGGL(k_ng_score, dim3(blocks(f)), dim3(256), 0, st, o, ws.key_a.p, ws.val_a.p);
        ANR_TRY(radix_sort_pairs_u64(ws.sort_temp.p, ws.key_a.p, ws.key_b.p, ws.val_a.p, ws.val_b.p, f, false, st));
        hipLaunchKernelGGL(k_ng_keys, dim3(blocks(f)), dim3(256), 0, st, o, ws.val_b.p, f, 0, ws.key_a.p);
        ANR_TRY(radix_sort_pairs_u64(ws.sort_temp.p, ws.key_a.p, ws.key_b.p, ws.val_b.p, ws.val_a.p, f, false, st));
        hipLaunchKernelGGL(k_ng_keys, dim3(blocks(f)), dim3(256), 0, st, o, ws.val_a.p, f, 1, ws.key_a.p);
        ANR_TRY(radix_sort_pairs_u64(ws.sort_temp.p, ws.key_a.p, ws.key_b.p, ws.val_a.p, ws.val_b.p, f, false, st));
        hipLaunchKernelGGL(k_ng_keys, dim3(blocks(f)), dim3(256), 0, st, o, ws.val_b.p, f, 2, ws.key_a.p);
        ANR_TRY(radix_sort_pairs_u64(ws.sort_temp.p, ws.key_a.p, ws.key_b.p, ws.val_b.p, ws.val_a.p, f, true, st));
        if (!host_out) {  // the best m again, by id
          hipLaunchKernelGGL(k_ng_keys, dim3(blocks(m)), dim3(256), 0, st, o, ws.val_a.p, m, 3, ws.key_a.p);
          ANR_TRY(radix_sort_pairs_u64(ws.sort_temp.p, ws.key_a.p, ws.key_b.p, ws.val_a.p, ws.val_b.p, m, false, st));
          perm = ws.val_b.p;
        }
      }
      if (host_out) {
        hipLaunchKernelGGL(k_ng_out_host, dim3(blocks(cap)), dim3(256), 0, st, o, perm, m, cap, ws.o_ids.p + (int64_t)ql * cap,
                           ws.o_dist.p + (int64_t)ql * cap, ws.o_score.p + (int64_t)ql * cap, ws.o_pos.p + (int64_t)ql * cap);
        out_count[q] = (int32_t)f;
      } else {
        hipLaunchKernelGGL(k_ng_out_dev, dim3(blocks(cap)), dim3(256), 0, st, o, perm, m, cap, ids_dev + q * cap,
                           scores_dev + q * cap, count_dev + q);
        if (out_count) out_count[q] = (int32_t)f;
      }
    }
    ANR_HIP(hipGetLastError());
    if (host_out) {
      const size_t cnt = (size_t)nqb * (size_t)cap;
      ANR_HIP(hipMemcpyAsync(out_ids + q0 * cap, ws.o_ids.p, cnt * 8, hipMemcpyDeviceToHost, st));
      if (out_dist) ANR_HIP(hipMemcpyAsync(out_dist + q0 * cap, ws.o_dist.p, cnt * 8, hipMemcpyDeviceToHost, st));
      if (out_score) ANR_HIP(hipMemcpyAsync(out_score + q0 * cap, ws.o_score.p, cnt * 8, hipMemcpyDeviceToHost, st));
      if (out_pos) ANR_HIP(hipMemcpyAsync(out_pos + q0 * cap, ws.o_pos.p, cnt * 4, hipMemcpyDeviceToHost, st));
    }
    ANR_HIP(hipStreamSynchronize(st));
  }
  return ANR_OK;
}

}  // namespace

extern "C" {

int anr_notegraph_create(int32_t device, int64_t n_nodes, int64_t n_edges, const int64_t *src, const int64_t *dst,
                         const double *w, anr_notegraph **out) {
  if (!out) return fail(ANR_EINVAL, "out is null");
  *out = nullptr;
  if (n_nodes < 1 || n_nodes >= 0x7fffffffll) return fail(ANR_EINVAL, "n_nodes must be in [1, 2^31 - 1)");
  if (n_edges < 0 || n_edges > (1ll << 30)) return fail(ANR_EINVAL, "n_edges must be in [0, 2^30]");
  if (n_edges > 0 && (!src || !dst || !w)) return fail(ANR_EINVAL, "null edge arrays");
  for (int64_t e = 0; e < n_edges; ++e) {
    if (src[e] < 0 || src[e] >= n_nodes || dst[e] < 0 || dst[e] >= n_nodes)
      return fail(ANR_EINVAL, "edge %lld: node id out of range", (long long)e);
    if (src[e] == dst[e]) return fail(ANR_EINVAL, "edge %lld: self-loop on node %lld", (long long)e, (long long)src[e]);
    if (!std::isfinite(w[e]) || w[e] < 0.0)
      return fail(ANR_EINVAL, "edge %lld: weight must be finite and non-negative", (long long)e);
  }
  int ndev = anr_device_count();
  if (ndev <= 0) return fail(ANR_EHIP, "no HIP device is visible");
  if (device < 0 || device >= ndev) return fail(ANR_EINVAL, "device %d out of range", device);
  DeviceGuard g(device);
  anr_notegraph *h = new anr_notegraph();
  h->device = device;
  h->n = n_nodes;
  h->E = n_edges;
  h->m = 2 * n_edges;
  const int64_t E = n_edges, m = h->m, n = n_nodes;
  int dup = 0;
  auto body = [&]() -> int {  // a failure destroys the handle below
    DevBuf<int64_t> d_src, d_dst;  // the build's buffers, of this call only
    DevBuf<double> d_w;
    DevBuf<u64> k0, k1;
    DevBuf<unsigned> v0, v1;
    DevBuf<unsigned char> temp;
    DevBuf<int> d_dup;
    ANR_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    hipStream_t st = h->stream;
    ANR_TRY(h->rowptr.alloc(n + 1, "note graph"));
    ANR_TRY(h->nbr.alloc(m, "note graph"));
    ANR_TRY(h->wt.alloc(m, "note graph"));
    ANR_TRY(h->cent.alloc(n, "note graph"));
    ANR_TRY(h->imp.alloc(n, "note graph"));
    ANR_HIP(hipMemsetAsync(h->cent.p, 0, (size_t)n * 8, st));
    hipLaunchKernelGGL(k_ng_fill_f64, dim3(blocks(n)), dim3(256), 0, st, h->imp.p, n, 1.0);
    ANR_TRY(d_dup.alloc(1, "note graph"));
    ANR_HIP(hipMemsetAsync(d_dup.p, 0, sizeof(int), st));
    if (E > 0) {
      ANR_TRY(d_src.alloc(E, "note graph"));
      ANR_TRY(d_dst.alloc(E, "note graph"));
      ANR_TRY(d_w.alloc(E, "note graph"));
      ANR_TRY(k0.alloc(m, "note graph"));
      ANR_TRY(k1.alloc(m, "note graph"));
      ANR_TRY(v0.alloc(m, "note graph"));
      ANR_TRY(v1.alloc(m, "note graph"));
      ANR_TRY(temp.alloc((int64_t)radix_sort_temp_bytes(m), "note graph"));
      ANR_HIP(hipMemcpyAsync(d_src.p, src, (size_t)E * 8, hipMemcpyHostToDevice, st));
      ANR_HIP(hipMemcpyAsync(d_dst.p, dst, (size_t)E * 8, hipMemcpyHostToDevice, st));
      ANR_HIP(hipMemcpyAsync(d_w.p, w, (size_t)E * 8, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(k_ng_edge_keys, dim3(blocks(m)), dim3(256), 0, st, d_src.p, d_dst.p, E, k0.p, v0.p);
      ANR_TRY(radix_sort_pairs_u64(temp.p, k0.p, k1.p, v0.p, v1.p, m, false, st));
      hipLaunchKernelGGL(k_ng_csr_fill, dim3(blocks(m)), dim3(256), 0, st, k1.p, v1.p, d_w.p, E, h->nbr.p, h->wt.p, d_dup.p);
    }
    hipLaunchKernelGGL(k_ng_rowptr, dim3(blocks(n + 1)), dim3(256), 0, st, k1.p, m, n, h->rowptr.p);
    ANR_HIP(hipGetLastError());
    ANR_HIP(hipMemcpyAsync(&dup, d_dup.p, sizeof(int), hipMemcpyDeviceToHost, st));
    ANR_HIP(hipStreamSynchronize(st));
    return ANR_OK;
  };
  int rc = body();
  if (rc == ANR_OK && dup) rc = fail(ANR_EINVAL, "an undirected pair is given more than once");
  if (rc != ANR_OK) {
    anr_notegraph_destroy(h);
    return rc;
  }
  *out = h;
  return ANR_OK;
}

int anr_notegraph_destroy(anr_notegraph *h) {
  if (!h) return ANR_OK;
  DeviceGuard g(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;  // frees the graph and both workspaces, still under the guard
  return ANR_OK;
}

int anr_notegraph_pagerank(anr_notegraph *h, double alpha, int32_t max_iter, double tol, double *out_host, int32_t *iters) {
  if (!h) return fail(ANR_EINVAL, "null handle");
  if (!(alpha >= 0.0 && alpha <= 1.0) || max_iter < 0 || !(tol >= 0.0)) return fail(ANR_EINVAL, "bad PageRank parameter");
  std::lock_guard<std::mutex> lk(h->mu);
  DeviceGuard g(h->device);
  hipStream_t st = h->stream;
  const int64_t n = h->n, m = h->m, nb = ceil_div(n, kNgChunk);
  int done = 0;
  bool converged = false;
  auto body = [&]() -> int {  // *iters is set below whatever comes of it
    DevBuf<double> b_inv, b_a, b_x, b_xn, b_part, b_scal;  // of this call
    ANR_TRY(b_inv.alloc(n, "note graph"));
    ANR_TRY(b_a.alloc(m, "note graph"));
    ANR_TRY(b_x.alloc(n, "note graph"));
    ANR_TRY(b_xn.alloc(n, "note graph"));
    ANR_TRY(b_part.alloc(2 * nb, "note graph"));
    ANR_TRY(b_scal.alloc(2, "note graph"));
    double *inv = b_inv.p, *a = b_a.p, *x = b_x.p, *xn = b_xn.p, *part = b_part.p, *scal = b_scal.p;  // x and xn swap
    const double p = 1.0 / (double)n;
    hipLaunchKernelGGL(k_ng_rowsum, dim3(blocks(n)), dim3(256), 0, st, h->rowptr.p, h->wt.p, n, inv);
    if (m > 0) hipLaunchKernelGGL(k_ng_scale, dim3(blocks(m)), dim3(256), 0, st, h->nbr.p, h->wt.p, inv, m, a);
    hipLaunchKernelGGL(k_ng_fill_f64, dim3(blocks(n)), dim3(256), 0, st, x, n, p);
    hipLaunchKernelGGL(k_ng_dangling, dim3((unsigned)nb), dim3(256), 0, st, x, inv, n, part + nb);
    hipLaunchKernelGGL(k_ng_final, dim3(1), dim3(256), 0, st, part + nb, nb, scal + 1);
    NgStep s{};
    s.rowptr = h->rowptr.p; s.nbr = h->nbr.p; s.a = a; s.inv = inv; s.scal = scal; s.part = part;
    s.alpha = alpha; s.p = p; s.omp = (1.0 - alpha) * p; s.n = n; s.nb = nb;
    for (int it = 0; it < max_iter && !converged; ++it) {
      s.x = x;
      s.xnew = xn;
      hipLaunchKernelGGL(k_ng_step, dim3((unsigned)nb), dim3(256), 0, st, s);
      hipLaunchKernelGGL(k_ng_final, dim3(2), dim3(256), 0, st, part, nb, scal);
      double err = 0.0;
      ANR_HIP(hipMemcpyAsync(&err, scal, 8, hipMemcpyDeviceToHost, st));
      ANR_HIP(hipStreamSynchronize(st));
      std::swap(x, xn);
      done = it + 1;
      converged = err < (double)n * tol;
    }
    ANR_HIP(hipGetLastError());
    if (converged) {
      ANR_HIP(hipMemcpyAsync(h->cent.p, x, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
      if (out_host) ANR_HIP(hipMemcpyAsync(out_host, x, (size_t)n * 8, hipMemcpyDeviceToHost, st));
      ANR_HIP(hipStreamSynchronize(st));
    }
    return ANR_OK;
  };
  const int rc = body();
  if (iters) *iters = done;
  if (rc != ANR_OK) return rc;
  if (!converged) return fail(ANR_ENOCONV, "PageRank did not converge within %d iterations", (int)max_iter);
  return ANR_OK;
}

int anr_notegraph_set_centrality(anr_notegraph *h, const double *c_host) {
  if (!h || !c_host) return fail(ANR_EINVAL, "bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  DeviceGuard g(h->device);
  ANR_HIP(hipMemcpyAsync(h->cent.p, c_host, (size_t)h->n * 8, hipMemcpyHostToDevice, h->stream));
  ANR_HIP(hipStreamSynchronize(h->stream));
  return ANR_OK;
}

int anr_notegraph_get_centrality(anr_notegraph *h, double *c_host) {
  if (!h || !c_host) return fail(ANR_EINVAL, "bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  DeviceGuard g(h->device);
  ANR_HIP(hipMemcpyAsync(c_host, h->cent.p, (size_t)h->n * 8, hipMemcpyDeviceToHost, h->stream));
  ANR_HIP(hipStreamSynchronize(h->stream));
  return ANR_OK;
}

int anr_notegraph_set_importance(anr_notegraph *h, const double *imp_host) {
  if (!h || !imp_host) return fail(ANR_EINVAL, "bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  DeviceGuard g(h->device);
  ANR_HIP(hipMemcpyAsync(h->imp.p, imp_host, (size_t)h->n * 8, hipMemcpyHostToDevice, h->stream));
  ANR_HIP(hipStreamSynchronize(h->stream));
  return ANR_OK;
}

int anr_notegraph_retrieve(anr_notegraph *h, int64_t nq, const int64_t *seed_offs, const int64_t *seeds, double cutoff,
                           int32_t cap, int64_t *out_ids, double *out_dist, double *out_score, int32_t *out_seed_pos,
                           int32_t *out_count) {
  ANR_TRY(check_seeds(h, nq, seed_offs, seeds, cutoff, cap));
  if (nq > 0 && (!out_ids || !out_count)) return fail(ANR_EINVAL, "null output");
  std::lock_guard<std::mutex> lk(h->mu);
  DeviceGuard g(h->device);
  int rc = retrieve_impl(h, nq, seed_offs, seeds, cutoff, cap, true, out_ids, out_dist, out_score, out_seed_pos, out_count,
                         nullptr, nullptr, nullptr);
  if (rc != ANR_OK) {  // a workspace left half-way does not hold its invariants: the next call builds a new one
    (void)hipStreamSynchronize(h->stream);
    free_workspace(h);
  }
  return rc;
}

int anr_notegraph_retrieve_dev(anr_notegraph *h, int64_t nq, const int64_t *seed_offs, const int64_t *seeds,
                               double cutoff, int32_t cap, uint32_t *ids_dev, double *scores_dev, int32_t *count_dev,
                               int32_t *out_found_host) {
  ANR_TRY(check_seeds(h, nq, seed_offs, seeds, cutoff, cap));
  if (cap > 65536) return fail(ANR_EINVAL, "cap must be <= 65536 (anr_fuse_source.sparse_cap)");
  if (nq > 0 && (!ids_dev || !scores_dev || !count_dev)) return fail(ANR_EINVAL, "null output");
  std::lock_guard<std::mutex> lk(h->mu);
  DeviceGuard g(h->device);
  int rc = retrieve_impl(h, nq, seed_offs, seeds, cutoff, cap, false, nullptr, nullptr, nullptr, nullptr, out_found_host,
                         ids_dev, scores_dev, count_dev);
  if (rc != ANR_OK) {
    (void)hipStreamSynchronize(h->stream);
    free_workspace(h);
  }
  return rc;
}

int anr_notegraph_rows_to_array_dev(anr_notegraph *h, int64_t nq, int32_t cap, const uint32_t *ids_dev,
                                    const double *scores_dev, const int32_t *count_dev, double *out_dev) {
  if (!h || nq < 0 || cap < 1) return fail(ANR_EINVAL, "bad argument");
  if (nq == 0) return ANR_OK;
  if (!ids_dev || !scores_dev || !count_dev || !out_dev) return fail(ANR_EINVAL, "null argument");
  if (nq > 65535) return fail(ANR_EINVAL, "at most 65535 queries per call");
  std::lock_guard<std::mutex> lk(h->mu);
  DeviceGuard g(h->device);
  hipStream_t st = h->stream;
  hipLaunchKernelGGL(k_ng_fill_f64, dim3(blocks(nq * h->n)), dim3(256), 0, st, out_dev, nq * h->n,
                     std::numeric_limits<double>::quiet_NaN());
  hipLaunchKernelGGL(k_ng_scatter_rows, dim3(blocks(cap), (unsigned)nq), dim3(256), 0, st, ids_dev, scores_dev, count_dev,
                     (int64_t)cap, h->n, out_dev);
  ANR_HIP(hipGetLastError());
  ANR_HIP(hipStreamSynchronize(st));
  return ANR_OK;
}

int anr_notegraph_components(anr_notegraph *h, int32_t *labels_host, int64_t *n_components) {
  if (!h || !labels_host) return fail(ANR_EINVAL, "bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  DeviceGuard g(h->device);
  hipStream_t st = h->stream;
  const int64_t n = h->n;
  ANR_TRY(ensure_quality_small(h));
  ANR_TRY(h->q_label.alloc(n, "note graph"));
  hipLaunchKernelGGL(k_ng_iota_i32, dim3(blocks(n)), dim3(256), 0, st, h->q_label.p, n);
  for (int changed = h->m > 0; changed;) {
    ANR_HIP(hipMemsetAsync(h->q_flag.p, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_ng_cc_hook, dim3(blocks(n * kNgLanes)), dim3(256), 0, st, h->rowptr.p, h->nbr.p, n, h->q_label.p,
                       h->q_flag.p);
    hipLaunchKernelGGL(k_ng_cc_flatten, dim3(blocks(n)), dim3(256), 0, st, h->q_label.p, n);
    ANR_HIP(hipGetLastError());
    ANR_HIP(hipMemcpyAsync(&changed, h->q_flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    ANR_HIP(hipStreamSynchronize(st));
  }
  u64 roots = 0;
  ANR_HIP(hipMemsetAsync(h->q_cnt.p + 2, 0, sizeof(u64), st));
  hipLaunchKernelGGL(k_ng_cc_roots, dim3(blocks(n)), dim3(256), 0, st, h->q_label.p, n, h->q_cnt.p + 2);
  ANR_HIP(hipGetLastError());
  ANR_HIP(hipMemcpyAsync(&roots, h->q_cnt.p + 2, sizeof(u64), hipMemcpyDeviceToHost, st));
  ANR_HIP(hipMemcpyAsync(labels_host, h->q_label.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  ANR_HIP(hipStreamSynchronize(st));
  if (n_components) *n_components = (int64_t)roots;
  return ANR_OK;
}

int anr_notegraph_hop_histogram(anr_notegraph *h, int64_t n_sources, const int64_t *sources, int64_t cap,
                                int64_t *counts_host, int64_t *n_levels, int64_t *stats8) {
  if (!h || cap < 0 || (cap > 0 && !counts_host)) return fail(ANR_EINVAL, "bad argument");
  if (n_levels) *n_levels = 0;
  const int64_t n = h->n;
  if (!sources) n_sources = n;
  if (n_sources < 0) return fail(ANR_EINVAL, "n_sources must be >= 0");
  std::vector<int32_t> src32;
  if (sources) {
    src32.resize((size_t)n_sources);
    for (int64_t j = 0; j < n_sources; ++j) {
      if (sources[j] < 0 || sources[j] >= n)
        return fail(ANR_EINVAL, "source %lld: node %lld out of range", (long long)j, (long long)sources[j]);
      src32[(size_t)j] = (int32_t)sources[j];
    }
  }
  std::lock_guard<std::mutex> lk(h->mu);
  DeviceGuard g(h->device);
  hipStream_t st = h->stream;
  ANR_TRY(ensure_quality_small(h));
  // words per node: the option or the default, halved while three state arrays do not fit half of the free memory
  int64_t W = h->bfs_words > 0 ? h->bfs_words : kNgBfsWords;
  if (h->q_state.cap < 3 * n * W) {
    h->q_state.release();
    size_t free_b = 0, total_b = 0;
    ANR_HIP(hipMemGetInfo(&free_b, &total_b));
    while (W > 1 && (size_t)(3 * n * W) * 8 > free_b / 2) W /= 2;
    ANR_TRY(h->q_state.alloc(3 * n * W, "note graph"));
  }
  if (sources && n_sources > 0) ANR_TRY(h->q_src.alloc(n_sources, "note graph"));
  if (sources && n_sources > 0)
    ANR_HIP(hipMemcpyAsync(h->q_src.p, src32.data(), (size_t)n_sources * sizeof(int32_t), hipMemcpyHostToDevice, st));
  const int64_t B = 64 * W, words = n * W;
  NgBfs p{};
  p.rowptr = h->rowptr.p; p.nbr = h->nbr.p; p.n = n; p.W = (int)W; p.cnt = h->q_cnt.p;
  while ((1 << p.wshift) < W) p.wshift += 1;
  p.seen = h->q_state.p;
  u64 *fa = h->q_state.p + words, *fb = h->q_state.p + 2 * words;
  std::vector<int64_t> counts;
  if (n_sources > 0) counts.push_back(n_sources);
  int64_t passes = 0, walked = 0;
  int slot = 0;
  Events<2> ev;  // the call's span on the stream, for stats8[6]
  if (stats8) ANR_TRY(ev.init());
  ANR_TRY(ev.mark(0, st));
  ANR_HIP(hipMemsetAsync(h->q_cnt.p, 0, 2 * sizeof(u64), st));
  for (int64_t s0 = 0; s0 < n_sources; s0 += B, ++passes) {
    p.base = s0;
    p.nbits = std::min<int64_t>(B, n_sources - s0);
    p.src = sources ? h->q_src.p + s0 : nullptr;
    ANR_HIP(hipMemsetAsync(p.seen, 0, (size_t)words * 8, st));
    ANR_HIP(hipMemsetAsync(fa, 0, (size_t)words * 8, st));
    hipLaunchKernelGGL(k_ng_bfs_seed, dim3(blocks(p.nbits)), dim3(256), 0, st, p, fa);
    u64 *fin = fa, *fout = fb;
    for (int64_t level = 1;; ++level) {
      p.fin = fin; p.fout = fout; p.slot = slot;
      hipLaunchKernelGGL(k_ng_bfs_level, dim3(blocks(words)), dim3(256), 0, st, p);
      ANR_HIP(hipGetLastError());
      u64 added = 0;
      ANR_HIP(hipMemcpyAsync(&added, h->q_cnt.p + slot, sizeof(u64), hipMemcpyDeviceToHost, st));
      ANR_HIP(hipStreamSynchronize(st));
      slot ^= 1;
      walked += 1;
      if (added == 0) break;
      if ((int64_t)counts.size() <= level) counts.resize((size_t)level + 1, 0);
      counts[(size_t)level] += (int64_t)added;
      std::swap(fin, fout);
    }
  }
  if (stats8) {
    float ms = 0.0f;
    ANR_TRY(ev.mark(1, st));
    ANR_HIP(hipEventSynchronize(ev.e[1]));
    ANR_TRY(ev.elapsed(0, 1, &ms));
    const int64_t st8[8] = {B, passes, walked, 3 * words * 8 + (sources ? n_sources * 4 : 0), W, n_sources,
                            (int64_t)((double)ms * 1000.0), 0};
    std::copy(st8, st8 + 8, stats8);
  }
  if (n_levels) *n_levels = (int64_t)counts.size();
  if ((int64_t)counts.size() > cap)
    return fail(ANR_EINVAL, "hop histogram: %lld levels do not fit cap = %lld", (long long)counts.size(), (long long)cap);
  for (int64_t l = 0; l < cap; ++l) counts_host[l] = l < (int64_t)counts.size() ? counts[(size_t)l] : 0;
  return ANR_OK;
}

int anr_notegraph_set_option(anr_notegraph *h, int32_t option, int64_t value) {
  if (!h) return fail(ANR_EINVAL, "null handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (option == ANR_NOTEGRAPH_OPT_MAX_SLOTS) {
    if (value < 0) return fail(ANR_EINVAL, "max slots must be >= 0");
    DeviceGuard g(h->device);
    (void)hipStreamSynchronize(h->stream);
    free_workspace(h);  // the next retrieve sizes it under the new bound
    h->max_slots = value;
    return ANR_OK;
  }
  if (option == ANR_NOTEGRAPH_OPT_BFS_WORDS) {
    if (value != 0 && value != 1 && value != 2 && value != 4 && value != 8 && value != 16)
      return fail(ANR_EINVAL, "BFS words per node must be 0 (default), 1, 2, 4, 8 or 16");
    DeviceGuard g(h->device);
    (void)hipStreamSynchronize(h->stream);
    h->q_state.release();  // the next hop histogram sizes it for the new width
    h->bfs_words = value;
    return ANR_OK;
  }
  return fail(ANR_EINVAL, "unknown note graph option %d", (int)option);
}

}  // extern "C"
