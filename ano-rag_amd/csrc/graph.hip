// Graph index on the exact index's handle: anr_index_graph_* (include/anorag.h), what reference
// vector_store/vector_index.py:94-99 builds as faiss.IndexHNSWFlat (one level, fixed out-degree R).  DESIGN.md §5d.
//
// Build (anr_index_graph_build):
//   knn   the handle's own exact streaming search over its stored rows, the queries device pointers into x32,
//         k = build_degree + 1; k_knn_lists drops the row's own id (when it is absent — un-normalised IP, where x.x is
//         not always the best score — the last entry instead).  Ties are ordered by ascending id, so the lists are
//         deterministic.
//   prune k_detour_order gives every list entry its rank-only detour count and orders the list stably by
//         (detour, rank) -> F; the host then adds reverse edges and cuts every list to R (rule in prune_host, restated
//         in tests/graph_ref.py).
//   image k_graph_image: a row-major int8 copy of x32 for the search's random row gathers — one power-of-two scale per
//         row, so that a code times a scale is exact (the scan images are MFMA-blocked: one row is 32-byte pieces 1 KiB
//         apart, wrong for gathers).
// Search (k_graph_search): one workgroup per query; a strided sample of up to 4096 rows seeds the beam, then a beam
// search over the graph with an LDS visited hash, then a float64 re-score of the beam from x32.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cfloat>
#include <vector>

#include "graph.hpp"

using namespace anr;

namespace {

constexpr int kMaxR = 128;       // out-degree
constexpr int kMaxK = 255;       // build_degree (k = build_degree + 1 of the kNN search <= 256)
constexpr int kMaxEf = 256;      // max(ef, k): the beam (itopk) is 64, 128 or 256 entries
constexpr int kMaxDim = 2048;
constexpr int kSortN = 512;      // beam + candidates, sorted together
constexpr int kCand = 256;       // candidates per iteration: p parents x R neighbours, p = 256 / R
constexpr int kHashBits = 12;
constexpr int kHash = 1 << kHashBits;  // visited hash slots; cleared when it would pass half full
constexpr int64_t kKnnChunk = 16384;   // queries per kNN search call
constexpr int64_t kEntry = 4096;       // entry sample: rows floor(i * n / S), i < S = min(n, kEntry), scored first
constexpr unsigned kIdMask = 0x7fffffffu;
constexpr unsigned kExpanded = 0x80000000u;
constexpr unsigned kNone = 0x7fffffffu;  // empty beam / candidate slot (carries kExpanded, so never a parent)

inline double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// ---------------------------------------------------------------------------------------------------------------------
// kernels

struct KnnListParams {
  const int64_t *I;  // [m][K + 1] the search's ids
  int64_t row0, m, id_offset;
  int K;
  int *lists;  // [n][K]
};

__global__ __launch_bounds__(256) void k_knn_lists(KnnListParams p) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= p.m) return;
  const int K1 = p.K + 1;
  const int64_t self = p.row0 + r + p.id_offset;
  const int64_t *src = p.I + r * K1;
  int *dst = p.lists + (p.row0 + r) * p.K;
  int skip = p.K;
  for (int j = 0; j < K1; ++j)
    if (src[j] == self) {
      skip = j;
      break;
    }
  int o = 0;
  for (int j = 0; j < K1; ++j) {
    if (j == skip) continue;
    const int64_t v = src[j];
    dst[o++] = v < 0 ? -1 : (int)(v - p.id_offset);
  }
}

__device__ __forceinline__ unsigned hash_slot(int id, int bits) { return ((unsigned)id * 2654435761u) >> (32 - bits); }

struct DetourParams {
  const int *lists;  // [n][K], valid ids first, -1 padding after them
  int64_t n;
  int K;
  int *F;  // [n][K]
};

// detour(i, r) = #{ s < r : L_i[r] is in L_{L_i[s]} at a position < r }; F_i = L_i stably sorted by (detour, r)
__global__ __launch_bounds__(256) void k_detour_order(DetourParams p) {
  __shared__ int s_L[256];
  __shared__ int s_hk[512], s_hv[512];  // id -> rank of the row's list
  __shared__ int s_det[256];
  const int t = threadIdx.x, K = p.K;
  const int64_t i = blockIdx.x;
  s_hk[t] = -1;
  s_hk[t + 256] = -1;
  s_det[t] = 0;
  const int v = t < K ? p.lists[i * K + t] : -1;
  s_L[t] = v;
  __syncthreads();
  if (v >= 0) {  // ids of one list are distinct
    unsigned s = hash_slot(v, 9);
    while (atomicCAS(&s_hk[s], -1, v) != -1) s = (s + 1) & 511;
    s_hv[s] = t;
  }
  __syncthreads();
  for (int e = t; e < K * K; e += 256) {
    const int s = e / K, u = e - s * K;
    const int ns = s_L[s];
    if (ns < 0 || s >= K - 1 || u >= K - 1) continue;
    const int m = p.lists[(int64_t)ns * K + u];
    if (m < 0) continue;
    unsigned h = hash_slot(m, 9);
    int r = -1;
    for (int key; (key = s_hk[h]) != -1; h = (h + 1) & 511)
      if (key == m) {
        r = s_hv[h];
        break;
      }
    if (r > s && r > u) atomicAdd(&s_det[r], 1);
  }
  __syncthreads();
  if (t < K) {
    int pos = t;  // padding keeps its place at the end
    if (v >= 0) {
      const int d = s_det[t];
      pos = 0;
      for (int r = 0; r < K; ++r) {
        if (s_L[r] < 0) continue;
        const int dr = s_det[r];
        pos += (dr < d || (dr == d && r < t)) ? 1 : 0;
      }
    }
    p.F[i * K + pos] = v;
  }
}

struct ImageParams {
  const float *x32;
  int64_t n;
  int dim, dimp;       // dimp: dim rounded up to 16 (row stride of the codes, one int4 per 16 values)
  signed char *codes;  // [n][dimp]
  int *rexp;           // [n] scale 2^rexp
  int *rsq;            // [n] sum of squared codes
};

// One wave per row.  Scale 2^(E - 7) with max|x| = m 2^E, m in [0.5, 1): codes rint(x / scale) in [-128, 128], clamped
// to +-127; a code times the scale is exact in float32, and so is every traversal score (k_graph_search).
__global__ __launch_bounds__(256) void k_graph_image(ImageParams p) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.n) return;
  const float *x = p.x32 + row * p.dim;
  float m = 0.0f;
  for (int c = lane; c < p.dim; c += 64) m = fmaxf(m, fabsf(x[c]));
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
  int e = 0;
  if (m > 0.0f) {
    int E;
    (void)frexpf(m, &E);
    e = E - 7;
  }
  int sq = 0;
  signed char *out = p.codes + row * p.dimp;
  for (int c = lane; c < p.dimp; c += 64) {
    const int v = c < p.dim ? (int)fminf(fmaxf(rintf(ldexpf(x[c], -e)), -127.0f), 127.0f) : 0;
    out[c] = (signed char)v;
    sq += v * v;
  }
  for (int off = 32; off > 0; off >>= 1) sq += __shfl_xor(sq, off);
  if (lane == 0) {
    p.rexp[row] = e;
    p.rsq[row] = sq;
  }
}

struct DecodeParams {
  const signed char *codes;
  const int *rexp;
  const int64_t *ids;  // device [n]
  int64_t n;
  int dim, dimp;
  float *out;  // [n][dim]
};

__global__ __launch_bounds__(256) void k_graph_decode(DecodeParams p) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= p.n * p.dim) return;
  const int64_t j = e / p.dim;
  const int c = (int)(e - j * p.dim);
  const int64_t id = p.ids[j];
  p.out[e] = ldexpf((float)p.codes[id * p.dimp + c], p.rexp[id]);
}

__device__ __forceinline__ int dot4(int a, int b, int c) {
  return c + (int)(signed char)a * (int)(signed char)b + ((a << 16) >> 24) * ((b << 16) >> 24) +
         ((a << 8) >> 24) * ((b << 8) >> 24) + (a >> 24) * (b >> 24);
}

// (key desc, id asc): the beam's total order
__device__ __forceinline__ bool before(double ka, unsigned ia, double kb, unsigned ib) {
  return ka > kb || (ka == kb && (ia & kIdMask) < (ib & kIdMask));
}

// bitonic sort of the kSortN (key, id) pairs in LDS, best first, 256 threads; callers synchronise before
__device__ void sort_pairs(double *key, unsigned *id) {
  const int t = threadIdx.x;
  for (int k2 = 2; k2 <= kSortN; k2 <<= 1)
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
      const int l = i + j;
      const double ka = key[i], kb = key[l];
      const unsigned ia = id[i], ib = id[l];
      const bool sw = (i & k2) == 0 ? before(kb, ib, ka, ia) : before(ka, ia, kb, ib);
      if (sw) {
        key[i] = kb;
        key[l] = ka;
        id[i] = ib;
        id[l] = ia;
      }
      __syncthreads();
    }
}

// true when id was not in the table (it is now); the table never passes half full (k_graph_search clears it first)
__device__ __forceinline__ bool visit(int *tab, int id, int *count) {
  unsigned s = hash_slot(id, kHashBits);
  for (;;) {
    const int old = atomicCAS(&tab[s], -1, id);
    if (old == -1) {
      atomicAdd(count, 1);
      return true;
    }
    if (old == id) return false;
    s = (s + 1) & (kHash - 1);
  }
}

struct SearchParams {
  const float *q;  // [nq][dim] as given (prepared here like k_prepq)
  const float *x32;
  const signed char *codes;
  const int *rexp, *rsq;
  const int *adj;  // [n][R]
  int64_t n, id_offset;
  int dim, dimp, R, k, efp, p, max_iter, metric, normalize;
  float *D;    // [nq][k]
  int64_t *I;  // [nq][k]
  int *qstat;  // [nq][3]: iterations, rows scored, stopped at max_iter
};

// Traversal key of row id, by a group of 16 lanes: the exact integer dot of the query codes and the row codes, times
// the two power-of-two scales (exact in float64); L2 ranks by 2 q.x - |x|^2 of the decoded vectors (= -|q - x|^2 up to
// the query's constant), one rounding.  Every lane of the group returns it.
__device__ __forceinline__ double trav_key(const SearchParams &p, const int *s_qc, int eq, int id, int sub) {
  const int4 *row = reinterpret_cast<const int4 *>(p.codes + (int64_t)id * p.dimp);
  int acc = 0;
  for (int c = sub; c < (p.dimp >> 4); c += 16) {
    const int4 w = row[c];
    acc = dot4(w.x, s_qc[4 * c], acc);
    acc = dot4(w.y, s_qc[4 * c + 1], acc);
    acc = dot4(w.z, s_qc[4 * c + 2], acc);
    acc = dot4(w.w, s_qc[4 * c + 3], acc);
  }
  for (int off = 8; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 16);
  const int er = p.rexp[id];
  if (p.metric == ANR_METRIC_IP) return ldexp((double)acc, eq + er);
  return ldexp((double)acc, eq + er + 1) - ldexp((double)p.rsq[id], 2 * er);
}

__device__ void score_slots(const SearchParams &p, const int *s_qc, int eq, double *key, const unsigned *id, int base,
                            int count) {
  const int g = threadIdx.x >> 4, sub = threadIdx.x & 15;
  for (int j = g; j < count; j += 16) {
    const unsigned v = id[base + j] & kIdMask;
    if (v == kNone) continue;
    const double kk = trav_key(p, s_qc, eq, (int)v, sub);
    if (sub == 0) key[base + j] = kk;
  }
}

// One workgroup per query.  LDS: query (f32 and int8 codes), beam + candidates (512 pairs), visited hash: ~32 KiB.
__global__ __launch_bounds__(256) void k_graph_search(SearchParams p) {
  __shared__ float s_q[kMaxDim];
  __shared__ int s_qc[kMaxDim / 4];
  __shared__ double s_key[kSortN];
  __shared__ unsigned s_id[kSortN];
  __shared__ int s_hash[kHash];
  __shared__ unsigned s_par[kCand];
  __shared__ double s_red[4];
  __shared__ float s_redf[4];
  __shared__ int s_wcnt[4];
  __shared__ int s_cnt[2];  // [0] visited entries in the hash, [1] rows scored
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t qi = blockIdx.x;
  const float *qin = p.q + qi * p.dim;

  // prepared query (k_prepq: divide by the float32 of the float64 norm) and its int8 codes (scale as k_graph_image)
  double acc = 0.0;
  for (int c = t; c < p.dim; c += 256) {
    const double v = (double)qin[c];
    acc += v * v;
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if (lane == 0) s_red[wave] = acc;
  __syncthreads();
  float scale = 1.0f;
  if (p.normalize) {
    const float nrm = (float)sqrt(s_red[0] + s_red[1] + s_red[2] + s_red[3]);
    if (nrm != 0.0f) scale = nrm;
  }
  float m = 0.0f;
  for (int c = t; c < p.dim; c += 256) {
    const float v = qin[c] / scale;
    s_q[c] = v;
    m = fmaxf(m, fabsf(v));
  }
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
  if (lane == 0) s_redf[wave] = m;
  for (int s = t; s < kHash; s += 256) s_hash[s] = -1;
  for (int s = t; s < kSortN; s += 256) {
    s_key[s] = -INFINITY;
    s_id[s] = kNone | kExpanded;
  }
  if (t < 2) s_cnt[t] = 0;
  __syncthreads();
  m = fmaxf(fmaxf(s_redf[0], s_redf[1]), fmaxf(s_redf[2], s_redf[3]));
  int eq = 0;
  if (m > 0.0f) {
    int E;
    (void)frexpf(m, &E);
    eq = E - 7;
  }
  for (int w = t; w < (p.dimp >> 2); w += 256) {
    unsigned packed = 0;
    for (int b = 0; b < 4; ++b) {
      const int c = 4 * w + b;
      const int v = c < p.dim ? (int)fminf(fmaxf(rintf(ldexpf(s_q[c], -eq)), -127.0f), 127.0f) : 0;
      packed |= ((unsigned)v & 0xffu) << (8 * b);
    }
    s_qc[w] = (int)packed;
  }

  // Entry: a fixed sample of S rows spread evenly over the corpus is scored kCand at a time and the best efp start the beam.  A one-level graph
  // built from exact kNN lists has no long edges: on a clustered corpus its clusters are barely linked, and a beam that
  // starts from efp rows (measured: recall@10 0.05-0.2 at 1 M rows in 1024 clusters) rarely reaches the query's one.
  // The sample plays the part of HNSW's upper levels.  Its rows are not put in the visited hash (only the beam's are,
  // below): one that comes back later is dropped again, as the comment on the iterations explains.
  const int efp = p.efp, R = p.R;
  const int64_t S = p.n < kEntry ? p.n : kEntry;
  __syncthreads();
  for (int64_t c0 = 0; c0 < S; c0 += kCand) {
    const int cnt = (int)(S - c0 < kCand ? S - c0 : kCand);
    for (int s = efp + t; s < kSortN; s += 256) {
      s_key[s] = -INFINITY;
      s_id[s] = kNone | kExpanded;
    }
    __syncthreads();
    if (t < cnt) s_id[efp + t] = (unsigned)((c0 + t) * p.n / S);
    __syncthreads();
    score_slots(p, s_qc, eq, s_key, s_id, efp, cnt);
    __syncthreads();
    sort_pairs(s_key, s_id);
  }
  if (t < efp && (s_id[t] & kIdMask) != kNone) visit(s_hash, (int)(s_id[t] & kIdMask), &s_cnt[0]);

  // Beam iterations.  The hash may forget: it is cleared when it would pass half full and refilled with the beam's ids,
  // so every id IN the beam is always in it and a candidate is never an id the beam already holds.  An id that was
  // forgotten had left the beam, i.e. its (key, id) fell below the beam's cut; the cut only rises, so when the id comes
  // back it is scored to the same key and dropped again.  The result is that of an exact visited set (what
  // tests/graph_ref.py restates); only the count of rows scored grows.
  int iters = 0, capped = 0;
  for (;;) {
    const bool f = t < efp && !(s_id[t] & kExpanded);
    const unsigned long long b = __ballot(f);
    if (lane == 0) s_wcnt[wave] = __popcll(b);
    __syncthreads();
    int below = 0, total = 0;
    for (int w = 0; w < 4; ++w) {
      below += w < wave ? s_wcnt[w] : 0;
      total += s_wcnt[w];
    }
    if (total == 0) break;
    if (iters == p.max_iter) {
      capped = 1;
      break;
    }
    const int np = total < p.p ? total : p.p;
    const bool reset = s_cnt[0] + np * R > kHash / 2;
    if (f) {
      const int rank = below + __popcll(b & ((1ull << lane) - 1ull));
      if (rank < p.p) {
        s_par[rank] = s_id[t] & kIdMask;
        s_id[t] |= kExpanded;
      }
    }
    ++iters;
    __syncthreads();
    if (reset) {
      for (int s = t; s < kHash; s += 256) s_hash[s] = -1;
      if (t == 0) s_cnt[0] = 0;
      __syncthreads();
      if (t < efp && (s_id[t] & kIdMask) != kNone) visit(s_hash, (int)(s_id[t] & kIdMask), &s_cnt[0]);
    }
    for (int s = efp + t; s < kSortN; s += 256) {
      s_key[s] = -INFINITY;
      s_id[s] = kNone | kExpanded;
    }
    __syncthreads();
    if (t < np * R) {
      const int nb = p.adj[(int64_t)s_par[t / R] * R + (t % R)];
      if (nb >= 0 && visit(s_hash, nb, &s_cnt[0])) {
        s_id[efp + t] = (unsigned)nb;
        atomicAdd(&s_cnt[1], 1);
      }
    }
    __syncthreads();
    score_slots(p, s_qc, eq, s_key, s_id, efp, np * R);
    __syncthreads();
    sort_pairs(s_key, s_id);
  }

  // float64 re-score of the beam from the stored rows; best k by (score, id)
  {
    const int g = t >> 4, sub = t & 15;
    for (int j = g; j < efp; j += 16) {
      const unsigned v = s_id[j] & kIdMask;
      if (v == kNone) continue;
      const float *x = p.x32 + (int64_t)v * p.dim;
      double a = 0.0;
      if (p.metric == ANR_METRIC_IP) {
        for (int c = sub; c < p.dim; c += 16) a += (double)s_q[c] * (double)x[c];
      } else {
        for (int c = sub; c < p.dim; c += 16) {
          const double d = (double)s_q[c] - (double)x[c];
          a += d * d;
        }
      }
      for (int off = 8; off > 0; off >>= 1) a += __shfl_xor(a, off, 16);
      if (sub == 0) s_key[j] = p.metric == ANR_METRIC_IP ? a : -a;
    }
    for (int s = efp + t; s < kSortN; s += 256) {
      s_key[s] = -INFINITY;
      s_id[s] = kNone | kExpanded;
    }
  }
  __syncthreads();
  sort_pairs(s_key, s_id);
  for (int j = t; j < p.k; j += 256) {
    const unsigned v = s_id[j] & kIdMask;
    const int64_t o = qi * p.k + j;
    if (v == kNone) {
      p.I[o] = -1;
      p.D[o] = p.metric == ANR_METRIC_IP ? -FLT_MAX : FLT_MAX;
    } else {
      p.I[o] = (int64_t)v + p.id_offset;
      p.D[o] = (float)(p.metric == ANR_METRIC_IP ? s_key[j] : -s_key[j]);
    }
  }
  if (t == 0) {
    p.qstat[qi * 3 + 0] = iters;
    p.qstat[qi * 3 + 1] = (int)S + s_cnt[1];
    p.qstat[qi * 3 + 2] = capped;
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// host side

struct anr_graph {
  std::mutex mu;                 // graph calls; taken before the index's own lock
  std::atomic<bool> stale{false};
  bool has = false;
  int R = 64, K = 128;           // of the current graph / the next rebuild
  int64_t n = 0;
  int dimp = 0;
  DevBuf<int> adj;            // device [n][R]
  DevBuf<signed char> codes;  // device [n][dimp]
  DevBuf<int> rexp, rsq;
  bool keep_knn = false;         // keep the pre-prune lists of every build (tests): n * K int32 of host memory
  std::vector<int> knn;          // host [n][K]: those lists (empty unless keep_knn, and after graph_set)
  // per-search scratch
  DevBuf<float> q, D;
  DevBuf<int64_t> I;
  DevBuf<int> qstat;
  std::vector<int> qstat_host;
  anr_graph_stats st{};
};

namespace anr {

void graph_mark_stale(anr_graph *g) {
  if (g) g->stale = true;
}

static void free_storage(anr_graph *g) {
  g->adj.release(), g->codes.release(), g->rexp.release(), g->rsq.release();
  g->has = false;
}

void graph_free(anr_graph *g) {
  delete g;  // on the index's device: anr_index_destroy calls this under its guard
}

}  // namespace anr

namespace {

anr_graph *graph_of(anr_index *h) {
  IndexCore c = index_core(h);
  std::lock_guard<std::mutex> lk(*c.mu);
  anr_graph *&g = index_graph(h);
  if (!g) g = new anr_graph();
  return g;
}

int check_dims(const IndexCore &c) {
  if (c.dim > kMaxDim) return fail(ANR_EINVAL, "the graph index takes dim <= %d (got %d)", kMaxDim, c.dim);
  if (c.ntotal > (int64_t)kIdMask - 1) return fail(ANR_EINVAL, "the graph index holds fewer than 2^31 - 1 rows");
  return ANR_OK;
}

// The final lists from F: first the first R/2 entries of F_i; then the rows j that have i among the first R/2 entries of
// F_j, in (position of i in F_j, j) order, skipping duplicates, up to R; then the rest of F_i, skipping duplicates; -1
// padding.
void prune_host(const std::vector<int> &F, int64_t n, int K, int R, std::vector<int> &adj) {
  const int half = std::min(R / 2, K);
  std::vector<int64_t> off(n + 1, 0);
  for (int64_t i = 0; i < n; ++i)
    for (int s = 0; s < half; ++s) {
      const int j = F[i * K + s];
      if (j >= 0) ++off[j + 1];
    }
  for (int64_t j = 0; j < n; ++j) off[j + 1] += off[j];
  std::vector<int> rev(off[n]);
  std::vector<int64_t> fill(off.begin(), off.end() - 1);
  for (int s = 0; s < half; ++s)
    for (int64_t i = 0; i < n; ++i) {
      const int j = F[i * K + s];
      if (j >= 0) rev[fill[j]++] = (int)i;
    }
  adj.assign(n * R, -1);
  std::vector<int> stamp(n, -1);
  for (int64_t i = 0; i < n; ++i) {
    int *out = adj.data() + i * R;
    int m = 0;
    auto take = [&](int v) {
      if (v >= 0 && m < R && stamp[v] != (int)i) {
        stamp[v] = (int)i;
        out[m++] = v;
      }
    };
    for (int s = 0; s < half; ++s) take(F[i * K + s]);
    for (int64_t e = off[i]; e < off[i + 1] && m < R; ++e) take(rev[e]);
    for (int s = half; s < K && m < R; ++s) take(F[i * K + s]);
  }
}

// the traversal image of the current rows (caller holds g->mu)
int build_image(anr_index *h, anr_graph *g) {
  IndexCore c = index_core(h);
  std::lock_guard<std::mutex> lk(*c.mu);
  const int64_t n = c.ntotal;
  g->dimp = (int)round_up(c.dim, 16);
  ANR_TRY(g->codes.alloc(n * g->dimp, "graph"));
  ANR_TRY(g->rexp.alloc(n, "graph"));
  ANR_TRY(g->rsq.alloc(n, "graph"));
  if (n > 0) {
    ImageParams ip{c.x32, n, c.dim, g->dimp, g->codes.p, g->rexp.p, g->rsq.p};
    hipLaunchKernelGGL(k_graph_image, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, c.stream, ip);
    ANR_HIP(hipGetLastError());
  }
  ANR_HIP(hipStreamSynchronize(c.stream));
  return ANR_OK;
}

// caller holds g->mu
int build_locked(anr_index *h, anr_graph *g, int R, int K) {
  IndexCore c = index_core(h);
  ANR_TRY(check_dims(c));
  const int64_t n = c.ntotal;
  free_storage(g);
  g->knn.clear();
  g->R = R;
  g->K = K;
  g->n = n;
  g->stale = false;
  auto t0 = std::chrono::steady_clock::now();
  // kNN lists: the exact streaming search of the index itself, chunk by chunk
  DevBuf<int> lists, F;  // these four are released before the graph itself is allocated
  DevBuf<float> Dk;
  DevBuf<int64_t> Ik;
  const int K1 = K + 1;
  const int64_t chunk = std::min<int64_t>(kKnnChunk, std::max<int64_t>(n, 1));
  int rc = lists.alloc(n * K, "graph");
  if (rc == ANR_OK) rc = F.alloc(n * K, "graph");
  if (rc == ANR_OK) rc = Dk.alloc(chunk * K1, "graph");
  if (rc == ANR_OK) rc = Ik.alloc(chunk * K1, "graph");
  for (int64_t i0 = 0; i0 < n && rc == ANR_OK; i0 += chunk) {
    const int64_t m = std::min(chunk, n - i0);
    rc = anr_index_search_dev_async(h, c.x32 + i0 * c.dim, m, K1, Dk.p, Ik.p, nullptr);
    if (rc == ANR_OK) rc = anr_index_sync(h);
    if (rc != ANR_OK) break;
    KnnListParams kp{Ik.p, i0, m, c.id_offset, K, lists.p};
    hipLaunchKernelGGL(k_knn_lists, dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, c.stream, kp);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    if (e != hipSuccess) rc = fail(ANR_EHIP, "kNN list kernel failed: %s", hipGetErrorString(e));
  }
  const double knn_ms = ms_since(t0);
  auto t1 = std::chrono::steady_clock::now();
  std::vector<int> Fh, adj;
  if (rc == ANR_OK && n > 0) {
    DetourParams dp{lists.p, n, K, F.p};
    hipLaunchKernelGGL(k_detour_order, dim3((unsigned)n), dim3(256), 0, c.stream, dp);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    Fh.resize(n * K);
    if (e == hipSuccess) e = hipMemcpy(Fh.data(), F.p, (size_t)n * K * sizeof(int), hipMemcpyDeviceToHost);
    if (g->keep_knn) {
      g->knn.resize(n * K);
      if (e == hipSuccess) e = hipMemcpy(g->knn.data(), lists.p, (size_t)n * K * sizeof(int), hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess) rc = fail(ANR_EHIP, "graph prune failed: %s", hipGetErrorString(e));
  }
  lists.release(), F.release(), Dk.release(), Ik.release();
  if (rc == ANR_OK) {
    prune_host(Fh, n, K, R, adj);
    Fh.clear();
    rc = g->adj.alloc(n * R, "graph");
    if (rc == ANR_OK && n > 0 &&
        hipMemcpy(g->adj.p, adj.data(), (size_t)n * R * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
      rc = fail(ANR_EHIP, "uploading the graph failed");
  }
  const double prune_ms = ms_since(t1);
  auto t2 = std::chrono::steady_clock::now();
  if (rc == ANR_OK) rc = build_image(h, g);
  if (rc != ANR_OK) {
    free_storage(g);
    g->knn.clear();
    return rc;
  }
  g->has = true;
  g->st.builds += 1;
  g->st.knn_ms = (float)knn_ms;
  g->st.prune_ms = (float)prune_ms;
  g->st.image_ms = (float)ms_since(t2);
  return ANR_OK;
}

// a graph that matches the rows: rebuilt when an add / reset came after it (caller holds g->mu)
int ensure_fresh(anr_index *h, anr_graph *g) {
  if (!g->has) return fail(ANR_ESTATE, "the index has no graph: call anr_index_graph_build first");
  if (g->stale || index_core(h).ntotal != g->n) return build_locked(h, g, g->R, g->K);
  return ANR_OK;
}

int search_impl(anr_index *h, const float *q, bool q_host, int64_t nq, int32_t k, int32_t ef, float *D, int64_t *I) {
  if (!h || (!q && nq > 0) || nq < 0 || !D || !I) return fail(ANR_EINVAL, "bad argument");
  if (k < 1 || ef < 1 || std::max(k, ef) > kMaxEf)
    return fail(ANR_EINVAL, "graph search needs 1 <= k, ef and max(k, ef) <= %d (got k %d, ef %d)", kMaxEf, k, ef);
  if (nq > 0x7fffffff) return fail(ANR_EINVAL, "too many queries");
  DeviceGuard dg(index_core(h).device);
  if (!dg.ok) return fail(ANR_EHIP, "hipSetDevice failed");
  anr_graph *g = graph_of(h);
  std::lock_guard<std::mutex> glk(g->mu);
  ANR_TRY(ensure_fresh(h, g));
  g->st.last_nq = nq;
  g->st.last_iterations = g->st.last_rows_scored = g->st.last_capped = 0;
  if (nq == 0) return ANR_OK;
  IndexCore c = index_core(h);
  const int64_t n = c.ntotal;
  if (n == 0) {
    for (int64_t e = 0; e < nq * k; ++e) {
      I[e] = -1;
      D[e] = c.metric == ANR_METRIC_IP ? -FLT_MAX : FLT_MAX;
    }
    return ANR_OK;
  }
  if (q_host) ANR_TRY(g->q.alloc(nq * c.dim, "graph"));
  ANR_TRY(g->D.alloc(nq * k, "graph"));
  ANR_TRY(g->I.alloc(nq * k, "graph"));
  ANR_TRY(g->qstat.alloc(nq * 3, "graph"));
  if (nq * 3 > (int64_t)g->qstat_host.size()) g->qstat_host.resize(nq * 3);
  std::lock_guard<std::mutex> lk(*c.mu);
  const float *qd = q;
  if (q_host) {
    ANR_HIP(hipMemcpyAsync(g->q.p, q, (size_t)nq * c.dim * sizeof(float), hipMemcpyHostToDevice, c.stream));
    qd = g->q.p;
  }
  int efp = 64;
  while (efp < std::max(k, ef)) efp <<= 1;
  SearchParams sp{};
  sp.q = qd;
  sp.x32 = c.x32;
  sp.codes = g->codes.p;
  sp.rexp = g->rexp.p;
  sp.rsq = g->rsq.p;
  sp.adj = g->adj.p;
  sp.n = n;
  sp.id_offset = c.id_offset;
  sp.dim = c.dim;
  sp.dimp = g->dimp;
  sp.R = g->R;
  sp.k = k;
  sp.efp = efp;
  sp.p = std::max(1, kCand / g->R);
  sp.max_iter = efp;
  sp.metric = c.metric;
  sp.normalize = c.normalize;
  sp.D = g->D.p;
  sp.I = g->I.p;
  sp.qstat = g->qstat.p;
  hipLaunchKernelGGL(k_graph_search, dim3((unsigned)nq), dim3(256), 0, c.stream, sp);
  ANR_HIP(hipGetLastError());
  ANR_HIP(hipMemcpyAsync(D, g->D.p, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, c.stream));
  ANR_HIP(hipMemcpyAsync(I, g->I.p, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost, c.stream));
  ANR_HIP(hipMemcpyAsync(g->qstat_host.data(), g->qstat.p, (size_t)nq * 3 * sizeof(int), hipMemcpyDeviceToHost, c.stream));
  ANR_HIP(hipStreamSynchronize(c.stream));
  for (int64_t i = 0; i < nq; ++i) {
    g->st.last_iterations += g->qstat_host[i * 3];
    g->st.last_rows_scored += g->qstat_host[i * 3 + 1];
    g->st.last_capped += g->qstat_host[i * 3 + 2];
  }
  return ANR_OK;
}

}  // namespace

extern "C" {

int anr_index_graph_build(anr_index *h, int32_t R, int32_t build_degree, int32_t keep_knn) {
  if (!h) return fail(ANR_EINVAL, "null handle");
  if (R < 2 || R > kMaxR || (R & 1)) return fail(ANR_EINVAL, "R must be even and in 2..%d (got %d)", kMaxR, R);
  if (build_degree < 1 || build_degree > kMaxK)
    return fail(ANR_EINVAL, "build_degree must be in 1..%d (got %d)", kMaxK, build_degree);
  DeviceGuard dg(index_core(h).device);
  if (!dg.ok) return fail(ANR_EHIP, "hipSetDevice failed");
  anr_graph *g = graph_of(h);
  std::lock_guard<std::mutex> glk(g->mu);
  g->keep_knn = keep_knn != 0;
  return build_locked(h, g, R, build_degree);
}

int anr_index_graph_search(anr_index *h, const float *q_host, int64_t nq, int32_t k, int32_t ef, float *D, int64_t *I) {
  return search_impl(h, q_host, true, nq, k, ef, D, I);
}

int anr_index_graph_search_devq(anr_index *h, const float *q_dev, int64_t nq, int32_t k, int32_t ef, float *D,
                                int64_t *I) {
  return search_impl(h, q_dev, false, nq, k, ef, D, I);
}

int anr_index_graph_get(anr_index *h, int32_t *adj, int64_t n, int32_t R) {
  if (!h || (!adj && n > 0)) return fail(ANR_EINVAL, "null argument");
  DeviceGuard dg(index_core(h).device);
  anr_graph *g = graph_of(h);
  std::lock_guard<std::mutex> glk(g->mu);
  ANR_TRY(ensure_fresh(h, g));
  if (n != g->n || R != g->R)
    return fail(ANR_EINVAL, "buffer of [%lld][%d] for a graph of [%lld][%d]", (long long)n, R, (long long)g->n, g->R);
  if (g->n > 0) ANR_HIP(hipMemcpy(adj, g->adj.p, (size_t)g->n * g->R * sizeof(int), hipMemcpyDeviceToHost));
  return ANR_OK;
}

int anr_index_graph_set(anr_index *h, const int32_t *adj, int64_t n, int32_t R) {
  if (!h || (!adj && n > 0)) return fail(ANR_EINVAL, "null argument");
  if (R < 2 || R > kMaxR || (R & 1)) return fail(ANR_EINVAL, "R must be even and in 2..%d (got %d)", kMaxR, R);
  IndexCore c = index_core(h);
  ANR_TRY(check_dims(c));
  if (n != c.ntotal) return fail(ANR_EINVAL, "graph of %lld rows for an index of %lld", (long long)n, (long long)c.ntotal);
  for (int64_t e = 0; e < n * R; ++e)
    if (adj[e] < -1 || adj[e] >= n) return fail(ANR_EINVAL, "graph entry %lld out of range", (long long)e);
  DeviceGuard dg(c.device);
  anr_graph *g = graph_of(h);
  std::lock_guard<std::mutex> glk(g->mu);
  free_storage(g);
  g->knn.clear();
  g->R = R;
  g->n = n;
  g->stale = false;
  ANR_TRY(g->adj.alloc(n * R, "graph"));
  if (n > 0) ANR_HIP(hipMemcpy(g->adj.p, adj, (size_t)n * R * sizeof(int), hipMemcpyHostToDevice));
  ANR_TRY(build_image(h, g));
  g->has = true;
  return ANR_OK;
}

int anr_index_graph_knn(anr_index *h, int32_t *lists, int64_t n, int32_t K) {
  if (!h || (!lists && n > 0)) return fail(ANR_EINVAL, "null argument");
  DeviceGuard dg(index_core(h).device);
  anr_graph *g = graph_of(h);
  std::lock_guard<std::mutex> glk(g->mu);
  ANR_TRY(ensure_fresh(h, g));
  if ((int64_t)g->knn.size() != g->n * g->K || (g->n > 0 && g->knn.empty()))
    return fail(ANR_ESTATE, "no kNN lists: the graph was set, or built without keep_knn");
  if (n != g->n || K != g->K)
    return fail(ANR_EINVAL, "buffer of [%lld][%d] for lists of [%lld][%d]", (long long)n, K, (long long)g->n, g->K);
  if (n > 0) std::memcpy(lists, g->knn.data(), g->knn.size() * sizeof(int));
  return ANR_OK;
}

int anr_index_graph_image(anr_index *h, const int64_t *ids, int64_t n, float *out) {
  if (!h || (n > 0 && (!ids || !out)) || n < 0) return fail(ANR_EINVAL, "bad argument");
  DeviceGuard dg(index_core(h).device);
  anr_graph *g = graph_of(h);
  std::lock_guard<std::mutex> glk(g->mu);
  ANR_TRY(ensure_fresh(h, g));
  for (int64_t j = 0; j < n; ++j)
    if (ids[j] < 0 || ids[j] >= g->n) return fail(ANR_EINVAL, "id %lld not in the index", (long long)ids[j]);
  if (n == 0) return ANR_OK;
  IndexCore c = index_core(h);
  DevBuf<int64_t> di;  // of this call
  DevBuf<float> dout;
  ANR_TRY(di.alloc(n, "graph"));
  ANR_TRY(dout.alloc(n * c.dim, "graph"));
  hipError_t e = hipMemcpy(di.p, ids, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice);
  DecodeParams dp{g->codes.p, g->rexp.p, di.p, n, c.dim, g->dimp, dout.p};
  if (e == hipSuccess)
    hipLaunchKernelGGL(k_graph_decode, dim3((unsigned)ceil_div(n * c.dim, 256)), dim3(256), 0, c.stream, dp);
  if (e == hipSuccess) e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
  if (e == hipSuccess) e = hipMemcpy(out, dout.p, (size_t)n * c.dim * sizeof(float), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(ANR_EHIP, "decoding the traversal image failed: %s", hipGetErrorString(e));
  return ANR_OK;
}

int anr_index_graph_stats(anr_index *h, anr_graph_stats *out) {
  if (!h || !out) return fail(ANR_EINVAL, "null argument");
  anr_graph *g = graph_of(h);
  std::lock_guard<std::mutex> glk(g->mu);
  *out = g->st;
  out->has_graph = g->has ? 1 : 0;
  out->stale = (g->stale || (g->has && index_core(h).ntotal != g->n)) ? 1 : 0;
  out->R = g->R;
  out->build_degree = g->K;
  out->graph_bytes = g->has ? g->n * g->R * (int64_t)sizeof(int) : 0;
  out->image_bytes = g->has ? g->n * (g->dimp + 2 * (int64_t)sizeof(int)) : 0;
  return ANR_OK;
}

}  // extern "C"
