// anr_index_khop_rerank and anr_index_cluster_suppress (include/anorag.h): the second hop of the reference's multi-hop
// query path for a batch of queries — _rerank_khop_candidates (query/query_processor.py:1549-1635) and
// _apply_cluster_suppression (:1637-1697).  k_khop_dot takes the dense and the focused cosine of every candidate from the
// index's stored rows; k_khop_rerank ranks, fuses and orders one query per workgroup.  k_khop_gram builds the upper
// triangle of one float64 Gram matrix per query with the shared tile (gram_f64.hpp); k_khop_suppress runs the greedy
// suppression on it, one workgroup per query.  DESIGN.md §5p has the layout, the order of operations and the error
// bound.  Compiled without multiply-add contraction (Makefile, EXACT).
#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>

#include "common.hpp"
#include "gram_f64.hpp"
#include "graph.hpp"

using namespace anr;

namespace {

constexpr int kMaxC = 1024;  // candidates per query
constexpr int kNT = 256;
constexpr int kTile = 32;    // a workgroup's tile of one query's Gram matrix: 2 x 2 waves of 16 x 16
constexpr int kLd = kGramKC + 1;

// ---------------------------------------------------------------------------------------------------------------------
// dense / focused: one wave per candidate.  Lane l sums the exact float64 products of k = l, l + 64, ... in ascending
// k; the 64 partial sums meet in a fixed butterfly (every lane ends with the same bits).  The value depends on the two
// vectors alone, never on the candidate's place in the batch.
struct KhopDot {
  const float *x32;
  int dim;
  const int64_t *rows;       // [total]
  const int *rowq;           // [total] query of a candidate
  const float *qv, *fv;      // [nq][dim]; fv may be nullptr
  const unsigned char *hasf; // [nq]; may be nullptr (no query has a focus)
  double *dense, *focused;   // [total]
  int total;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off);
  return v;
}

__device__ __forceinline__ double cos_clamped(double dot, double na, double nb) {
  if (na == 0.0 || nb == 0.0) return 0.0;
  const double s = dot / (na * nb);
  return s > 0.0 ? s : 0.0;  // Python's max(0.0, s)
}

__global__ __launch_bounds__(kNT) void k_khop_dot(KhopDot p) {
  const int lane = threadIdx.x & 63;
  const int c = (int)blockIdx.x * (kNT / 64) + (threadIdx.x >> 6);
  if (c >= p.total) return;  // whole waves leave: no barrier below
  const int q = p.rowq[c];
  const float *x = p.x32 + p.rows[c] * p.dim;
  const float *qv = p.qv + (int64_t)q * p.dim;
  const bool foc = p.fv && p.hasf && p.hasf[q];
  const float *fv = foc ? p.fv + (int64_t)q * p.dim : qv;
  double xx = 0.0, qq = 0.0, qx = 0.0, ff = 0.0, fx = 0.0;
  for (int k = lane; k < p.dim; k += 64) {
    const double xv = (double)x[k], a = (double)qv[k];
    xx += xv * xv;
    qq += a * a;
    qx += a * xv;
    if (foc) {
      const double b = (double)fv[k];
      ff += b * b;
      fx += b * xv;
    }
  }
  xx = wave_sum(xx), qq = wave_sum(qq), qx = wave_sum(qx);
  ff = wave_sum(ff), fx = wave_sum(fx);
  if (lane == 0) {
    const double nx = sqrt(xx);
    p.dense[c] = cos_clamped(qx, sqrt(qq), nx);
    p.focused[c] = foc ? cos_clamped(fx, sqrt(ff), nx) : 0.0;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
struct KhopRerank {
  const int64_t *offs;
  const double *dense, *focused, *bm25, *prf_sim, *cov, *decay;
  const unsigned char *is_prf;
  const int *cons, *hop_no;
  anr_khop_params prm;
  double *fin;
  int *order;
};

// 1-based rank of entry c among n by s descending, ties in candidate order
__device__ __forceinline__ int rank_desc(const double *s, int n, int c) {
  const double sc = s[c];
  int r = 1;
  for (int j = 0; j < n; ++j) {
    const double sj = s[j];
    r += (sj > sc || (sj == sc && j < c)) ? 1 : 0;
  }
  return r;
}

// One query: the three rankings by counting, the RRF bonus, the final score, the stable order.  Threads own candidates
// (strided); every loop is bounded by C.
__global__ __launch_bounds__(kNT) void k_khop_rerank(KhopRerank a) {
  __shared__ double sd[kMaxC], sb[kMaxC], sp[kMaxC], sf[kMaxC];
  __shared__ unsigned char prf[kMaxC];
  const int q = blockIdx.x, tid = threadIdx.x;
  const int64_t o = a.offs[q];
  const int C = (int)(a.offs[q + 1] - o);
  if (C == 0) return;
  for (int c = tid; c < C; c += kNT) {
    sd[c] = a.dense[o + c];
    sb[c] = a.bm25[o + c];
    sp[c] = a.prf_sim[o + c];
    prf[c] = a.is_prf[o + c] ? 1 : 0;
  }
  __syncthreads();
  const anr_khop_params &w = a.prm;
  for (int c = tid; c < C; c += kNT) {
    // the three rankings in one pass over the list: entries ahead of c by score descending, ties in candidate order
    const double dc = sd[c], bc = sb[c], pc = sp[c];
    int rd = 1, rb = 1, rp = 1;
    for (int j = 0; j < C; ++j) {
      const double dj = sd[j], bj = sb[j], pj = sp[j];
      rd += (dj > dc || (dj == dc && j < c)) ? 1 : 0;
      rb += (bj > bc || (bj == bc && j < c)) ? 1 : 0;
      rp += (prf[j] && (pj > pc || (pj == pc && j < c))) ? 1 : 0;
    }
    double rrf = (0.0 + 1.0 / (w.rrf_k + (double)rd)) + 1.0 / (w.rrf_k + (double)rb);  // _rrf_score: dense, bm25, prf
    if (prf[c]) rrf = rrf + 1.0 / (w.rrf_k + (double)rp);
    const int hop = a.hop_no[o + c];
    double fw = w.focused_w2;
    if (hop != 2) {
      fw = w.focused_w2 - 0.10 * ((double)hop - 2.0);
      fw = fw > 0.0 ? fw : 0.0;  // max(0.0, .)
    }
    const double base = w.dense_w * sd[c] + w.bm25_w * sb[c];
    double fin = (((base + fw * a.focused[o + c]) + w.cov_w * a.cov[o + c]) + w.cons_w * (double)a.cons[o + c]) + w.rrf_lambda * rrf;
    fin = fin * a.decay[o + c];
    sf[c] = fin;
    a.fin[o + c] = fin;
  }
  __syncthreads();
  for (int c = tid; c < C; c += kNT) a.order[o + rank_desc(sf, C, c) - 1] = c;
}

// ---------------------------------------------------------------------------------------------------------------------
struct KhopGram {
  const float *x32;
  int dim;
  const int64_t *rows, *offs, *soff;
  const int *tiles;  // [n_tiles][3]: query, tile row, tile column (row <= column)
  double *G;         // the upper triangle (j >= i) of every query's C x C block is written
  double *nrm;       // [total] sqrt(G_ii)
};

// Raw products of one 32 x 32 tile, as k_div_gram (diversity.hip) walks them; nothing below the diagonal is written.
__global__ __launch_bounds__(kNT) void k_khop_gram(KhopGram p) {
  __shared__ float As[kTile][kLd], Bs[kTile][kLd];
  __shared__ int64_t ra[kTile], rb[kTile];
  const int q = p.tiles[3 * blockIdx.x], bi = p.tiles[3 * blockIdx.x + 1], bj = p.tiles[3 * blockIdx.x + 2];
  const int64_t o = p.offs[q];
  const int C = (int)(p.offs[q + 1] - o);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wi = w >> 1, wj = w & 1;
  if (tid < kTile) {
    const int ia = bi * kTile + tid, ib = bj * kTile + tid;
    ra[tid] = ia < C ? p.rows[o + ia] : -1;
    rb[tid] = ib < C ? p.rows[o + ib] : -1;
  }
  __syncthreads();
  double4_t acc[1];
  gram_f64_tile<2, 2, 1, kLd>(p.x32, p.dim, ra, rb, As, Bs, acc);
  double *G = p.G + p.soff[q];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = bi * kTile + wi * 16 + (lane >> 4) + 4 * r, j = bj * kTile + wj * 16 + (lane & 15);
    if (i < C && j < C && j >= i) {
      G[(int64_t)i * C + j] = acc[0][r];
      if (i == j) p.nrm[o + i] = sqrt(acc[0][r]);
    }
  }
}

struct KhopSuppress {
  const double *sim;   // raw: the Gram's upper triangle; else the caller's cosines
  const double *nrm;   // raw only
  const int64_t *offs, *soff;
  const double *score;
  double thr;
  int keep_m, raw;
  int *kept, *n_kept;
};

// The reference's loop of one query (:1671-1693).  Threads own candidates (strided).  A seed's later members are
// collected in LDS through an integer counter; their order there does not matter, the cluster's stable sort is a count
// over (score, position).  A seed without a later member costs one barrier.  The seed test and every count are read from
// LDS after a barrier, so every branch is taken by the whole workgroup.
__global__ __launch_bounds__(kNT) void k_khop_suppress(KhopSuppress a) {
  __shared__ double sc[kMaxC], ks[kMaxC];
  __shared__ int klist[kMaxC], clist[kMaxC];
  __shared__ unsigned char used[kMaxC];
  __shared__ int s_cnt[3];  // a seed step counts in s_cnt[step % 3]; the next step's counter is cleared one barrier ahead
  const int q = blockIdx.x, tid = threadIdx.x;
  const int64_t o = a.offs[q];
  const int C = (int)(a.offs[q + 1] - o);
  if (C == 0) {
    if (tid == 0) a.n_kept[q] = 0;
    return;
  }
  const double *sim = a.sim + a.soff[q];
  for (int c = tid; c < C; c += kNT) {
    sc[c] = a.score[o + c];
    used[c] = 0;
  }
  if (tid < 3) s_cnt[tid] = 0;
  __syncthreads();
  int nk = 0, step = 0;
  for (int i = 0; i < C; ++i) {
    if (used[i]) continue;  // uniform: written before the closing barrier of an earlier step
    int *cnt = &s_cnt[step % 3];
    if (tid == 0) s_cnt[(step + 1) % 3] = 0;  // last read two barriers ago
    ++step;
    const double *row = sim + (int64_t)i * C;
    const double di = a.raw ? a.nrm[o + i] + 1e-8 : 1.0;
    for (int j = i + 1 + tid; j < C; j += kNT) {
      if (used[j]) continue;
      double s = row[j];
      if (a.raw) s = s / (di * (a.nrm[o + j] + 1e-8));
      if (s >= a.thr) clist[atomicAdd(cnt, 1)] = j;
    }
    __syncthreads();
    const int n = *cnt;  // later members; the cluster is the seed and these
    if (n == 0) {
      if (tid == 0) klist[nk] = i;  // keep_m >= 1; used[i] is never read again
      nk += 1;
      continue;
    }
    // the cluster's stable sort by score descending (the reference's list is in ascending position), by counting; its
    // first keep_m are appended
    for (int t = tid; t <= n; t += kNT) {
      const int j = t == n ? i : clist[t];
      const double sj = sc[j];
      int r = (sc[i] > sj || (sc[i] == sj && i < j)) ? 1 : 0;
      for (int e = 0; e < n; ++e) {
        const int m = clist[e];
        const double sm = sc[m];
        r += (sm > sj || (sm == sj && m < j)) ? 1 : 0;
      }
      if (r < a.keep_m) klist[nk + r] = j;
      used[j] = 1;
    }
    nk += n + 1 < a.keep_m ? n + 1 : a.keep_m;
    __syncthreads();  // used[] and clist before the next seed
  }
  __syncthreads();
  // the kept list, stably sorted by score descending
  for (int p = tid; p < nk; p += kNT) ks[p] = sc[klist[p]];
  __syncthreads();
  for (int p = tid; p < nk; p += kNT) {
    const double s = ks[p];
    int r = 0;
    for (int m = 0; m < nk; ++m) r += (ks[m] > s || (ks[m] == s && m < p)) ? 1 : 0;
    a.kept[o + r] = klist[p];
  }
  if (tid == 0) a.n_kept[q] = nk;
}

// developer timing (anr_khop_timing): HIP-event times of the last timed calls
bool g_timing = false;
float g_times[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

bool is_nan(double v) { return !(v == v); }

// offs ascends from 0 and no list is longer than the limit
int check_offs(const char *what, int64_t nq, const int64_t *offs) {
  if (offs[0] != 0) return fail(ANR_EINVAL, "%s: offs must start at 0", what);
  for (int64_t q = 0; q < nq; ++q) {
    const int64_t C = offs[q + 1] - offs[q];
    if (C < 0) return fail(ANR_EINVAL, "%s: offs must ascend", what);
    if (C > kMaxC)
      return fail(ANR_EINVAL, "%s: query %lld has %lld candidates (limit %d)", what, (long long)q, (long long)C, kMaxC);
  }
  if (nq > 0x7fffffffLL || offs[nq] > 0x7fffffffLL) return fail(ANR_EINVAL, "%s: too many queries or candidates for one call", what);
  return ANR_OK;
}

int check_numbers(const char *what, const char *name, const double *v, int64_t n) {
  for (int64_t e = 0; e < n; ++e)
    if (is_nan(v[e])) return fail(ANR_EINVAL, "%s: %s[%lld] is not a number", what, name, (long long)e);
  return ANR_OK;
}

int check_rows(const char *what, const int64_t *rows, int64_t n, int64_t ntotal) {
  for (int64_t e = 0; e < n; ++e)
    if (rows[e] < 0 || rows[e] >= ntotal)
      return fail(ANR_EINVAL, "%s: row id %lld outside [0, %lld)", what, (long long)rows[e], (long long)ntotal);
  return ANR_OK;
}

struct RerankArgs {
  int64_t nq;
  const int64_t *offs, *rows;
  const float *qv, *fv;
  const uint8_t *hasf;
  const double *dense_in, *focused_in, *bm25, *prf_sim, *cov, *decay;
  const uint8_t *is_prf;
  const int32_t *cons, *hop_no;
  anr_khop_params prm;
  double *dense, *focused, *fin;
  int32_t *order;
};

int run_rerank(DevBuf<unsigned char> &arena, const float *x32, int dim, const RerankArgs &r, hipStream_t st) {
  const int64_t nq = r.nq, total = r.offs[nq];
  const bool given = r.dense_in != nullptr;
  ArenaLayout<8> lay;
  const size_t o_offs = lay.take((size_t)(nq + 1) * 8);
  const size_t o_bm25 = lay.take((size_t)total * 8), o_prf = lay.take((size_t)total * 8), o_cov = lay.take((size_t)total * 8);
  const size_t o_decay = lay.take((size_t)total * 8);
  const size_t o_cons = lay.take((size_t)total * 4), o_hop = lay.take((size_t)total * 4), o_isprf = lay.take((size_t)total);
  const size_t o_rows = lay.take(given ? 0 : (size_t)total * 8), o_rowq = lay.take(given ? 0 : (size_t)total * 4);
  const size_t o_qv = lay.take(given ? 0 : (size_t)nq * dim * 4), o_fv = lay.take(given || !r.fv ? 0 : (size_t)nq * dim * 4);
  const size_t o_hasf = lay.take(given || !r.hasf ? 0 : (size_t)nq);
  const size_t in_end = lay.at;
  // outputs, one copy back; the given dense / focused are uploaded into the same two arrays
  const size_t o_dense = lay.take((size_t)total * 8), o_foc = lay.take((size_t)total * 8), o_fin = lay.take((size_t)total * 8);
  const size_t o_order = lay.take((size_t)total * 4);
  const size_t out_end = lay.at;
  ANR_TRY(arena.alloc((int64_t)out_end, "khop_rerank", (int64_t)(out_end + out_end / 4), "the candidate arrays"));
  unsigned char *A = arena.p;

  std::vector<unsigned char> in(given ? o_foc + (size_t)total * 8 : in_end, 0);
  memcpy(&in[o_offs], r.offs, (size_t)(nq + 1) * 8);
  memcpy(&in[o_bm25], r.bm25, (size_t)total * 8);
  memcpy(&in[o_prf], r.prf_sim, (size_t)total * 8);
  memcpy(&in[o_cov], r.cov, (size_t)total * 8);
  memcpy(&in[o_decay], r.decay, (size_t)total * 8);
  memcpy(&in[o_cons], r.cons, (size_t)total * 4);
  memcpy(&in[o_hop], r.hop_no, (size_t)total * 4);
  memcpy(&in[o_isprf], r.is_prf, (size_t)total);
  if (given) {
    memcpy(&in[o_dense], r.dense_in, (size_t)total * 8);
    if (r.focused_in) memcpy(&in[o_foc], r.focused_in, (size_t)total * 8);  // else zeros
  } else {
    memcpy(&in[o_rows], r.rows, (size_t)total * 8);
    int *rowq = reinterpret_cast<int *>(&in[o_rowq]);
    for (int64_t q = 0; q < nq; ++q)
      for (int64_t c = r.offs[q]; c < r.offs[q + 1]; ++c) rowq[c] = (int)q;
    memcpy(&in[o_qv], r.qv, (size_t)nq * dim * 4);
    if (r.fv) memcpy(&in[o_fv], r.fv, (size_t)nq * dim * 4);
    if (r.hasf) memcpy(&in[o_hasf], r.hasf, (size_t)nq);
  }
  Events<4> ev;
  if (g_timing) ANR_TRY(ev.init());
  ANR_TRY(ev.mark(0, st));
  ANR_HIP(hipMemcpyAsync(A, in.data(), in.size(), hipMemcpyHostToDevice, st));
  double *dense = reinterpret_cast<double *>(A + o_dense), *foc = reinterpret_cast<double *>(A + o_foc);
  ANR_TRY(ev.mark(1, st));
  if (!given) {
    KhopDot d{x32,
              dim,
              reinterpret_cast<const int64_t *>(A + o_rows),
              reinterpret_cast<const int *>(A + o_rowq),
              reinterpret_cast<const float *>(A + o_qv),
              r.fv ? reinterpret_cast<const float *>(A + o_fv) : nullptr,
              r.hasf ? A + o_hasf : nullptr,
              dense,
              foc,
              (int)total};
    hipLaunchKernelGGL(k_khop_dot, dim3((unsigned)ceil_div(total, kNT / 64)), dim3(kNT), 0, st, d);
    ANR_HIP(hipGetLastError());
  }
  ANR_TRY(ev.mark(2, st));
  KhopRerank k{};
  k.offs = reinterpret_cast<const int64_t *>(A + o_offs);
  k.dense = dense;
  k.focused = foc;
  k.bm25 = reinterpret_cast<const double *>(A + o_bm25);
  k.prf_sim = reinterpret_cast<const double *>(A + o_prf);
  k.cov = reinterpret_cast<const double *>(A + o_cov);
  k.decay = reinterpret_cast<const double *>(A + o_decay);
  k.is_prf = A + o_isprf;
  k.cons = reinterpret_cast<const int *>(A + o_cons);
  k.hop_no = reinterpret_cast<const int *>(A + o_hop);
  k.prm = r.prm;
  k.fin = reinterpret_cast<double *>(A + o_fin);
  k.order = reinterpret_cast<int *>(A + o_order);
  hipLaunchKernelGGL(k_khop_rerank, dim3((unsigned)nq), dim3(kNT), 0, st, k);
  ANR_HIP(hipGetLastError());
  ANR_TRY(ev.mark(3, st));
  std::vector<unsigned char> out(out_end - o_dense);
  ANR_HIP(hipMemcpyAsync(out.data(), A + o_dense, out.size(), hipMemcpyDeviceToHost, st));
  ANR_HIP(hipStreamSynchronize(st));
  if (ev.on) {
    ANR_TRY(ev.elapsed(1, 2, &g_times[0]));
    ANR_TRY(ev.elapsed(2, 3, &g_times[1]));
    ANR_TRY(ev.elapsed(0, 3, &g_times[2]));
  }
  const unsigned char *O = out.data() - o_dense;
  if (r.dense) memcpy(r.dense, O + o_dense, (size_t)total * 8);
  if (r.focused) memcpy(r.focused, O + o_foc, (size_t)total * 8);
  if (r.fin) memcpy(r.fin, O + o_fin, (size_t)total * 8);
  if (r.order) memcpy(r.order, O + o_order, (size_t)total * 4);
  return ANR_OK;
}

int run_suppress(DevBuf<unsigned char> &sim_buf, DevBuf<unsigned char> &arena, const float *x32, int dim, int64_t nq,
                 const int64_t *offs, const int64_t *rows, const double *sim_host, const double *score, double thr,
                 int keep_m, int32_t *kept, int32_t *n_kept, hipStream_t st) {
  const int64_t total = offs[nq];
  std::vector<int64_t> soff((size_t)nq);
  std::vector<int> tiles;
  int64_t stotal = 0;
  for (int64_t q = 0; q < nq; ++q) {
    const int64_t C = offs[q + 1] - offs[q];
    soff[q] = stotal;
    stotal += C * C;
    if (!sim_host) {
      const int nb = (int)ceil_div(C, kTile);
      for (int bi = 0; bi < nb; ++bi)
        for (int bj = bi; bj < nb; ++bj) {
          tiles.push_back((int)q);
          tiles.push_back(bi);
          tiles.push_back(bj);
        }
    }
  }
  const int64_t n_tiles = (int64_t)tiles.size() / 3;
  if (n_tiles > 0x7fffffffLL) return fail(ANR_EINVAL, "cluster_suppress: too many candidates for one call");
  ArenaLayout<8> lay;
  const size_t o_offs = lay.take((size_t)(nq + 1) * 8), o_soff = lay.take((size_t)nq * 8), o_score = lay.take((size_t)total * 8);
  const size_t o_rows = lay.take(sim_host ? 0 : (size_t)total * 8), o_tiles = lay.take(tiles.size() * 4);
  const size_t in_end = lay.at;
  const size_t o_nrm = lay.take((size_t)total * 8);
  const size_t o_kept = lay.take((size_t)total * 4), o_nk = lay.take((size_t)nq * 4);
  const size_t out_end = lay.at;
  ANR_TRY(arena.alloc((int64_t)out_end, "cluster_suppress", (int64_t)(out_end + out_end / 4), "the candidate arrays"));
  ANR_TRY(sim_buf.alloc(stotal * 8, "cluster_suppress", stotal * 10, "the similarity matrices"));
  unsigned char *A = arena.p;
  double *sim = reinterpret_cast<double *>(sim_buf.p);

  std::vector<unsigned char> in(in_end, 0);
  memcpy(&in[o_offs], offs, (size_t)(nq + 1) * 8);
  memcpy(&in[o_soff], soff.data(), (size_t)nq * 8);
  memcpy(&in[o_score], score, (size_t)total * 8);
  if (!sim_host) {
    memcpy(&in[o_rows], rows, (size_t)total * 8);
    if (!tiles.empty()) memcpy(&in[o_tiles], tiles.data(), tiles.size() * 4);
  }
  Events<4> ev;
  if (g_timing) ANR_TRY(ev.init());
  ANR_TRY(ev.mark(0, st));
  ANR_HIP(hipMemcpyAsync(A, in.data(), in_end, hipMemcpyHostToDevice, st));
  ANR_TRY(ev.mark(1, st));
  if (sim_host) {
    ANR_HIP(hipMemcpyAsync(sim, sim_host, (size_t)stotal * 8, hipMemcpyHostToDevice, st));
  } else {
    KhopGram g{x32,
               dim,
               reinterpret_cast<const int64_t *>(A + o_rows),
               reinterpret_cast<const int64_t *>(A + o_offs),
               reinterpret_cast<const int64_t *>(A + o_soff),
               reinterpret_cast<const int *>(A + o_tiles),
               sim,
               reinterpret_cast<double *>(A + o_nrm)};
    hipLaunchKernelGGL(k_khop_gram, dim3((unsigned)n_tiles), dim3(kNT), 0, st, g);
    ANR_HIP(hipGetLastError());
  }
  ANR_TRY(ev.mark(2, st));
  KhopSuppress s{};
  s.sim = sim;
  s.nrm = reinterpret_cast<const double *>(A + o_nrm);
  s.offs = reinterpret_cast<const int64_t *>(A + o_offs);
  s.soff = reinterpret_cast<const int64_t *>(A + o_soff);
  s.score = reinterpret_cast<const double *>(A + o_score);
  s.thr = thr;
  s.keep_m = keep_m;
  s.raw = sim_host ? 0 : 1;
  s.kept = reinterpret_cast<int *>(A + o_kept);
  s.n_kept = reinterpret_cast<int *>(A + o_nk);
  hipLaunchKernelGGL(k_khop_suppress, dim3((unsigned)nq), dim3(kNT), 0, st, s);
  ANR_HIP(hipGetLastError());
  ANR_TRY(ev.mark(3, st));
  std::vector<unsigned char> out(out_end - o_kept);
  ANR_HIP(hipMemcpyAsync(out.data(), A + o_kept, out.size(), hipMemcpyDeviceToHost, st));
  ANR_HIP(hipStreamSynchronize(st));
  if (ev.on) {
    ANR_TRY(ev.elapsed(1, 2, &g_times[3]));
    ANR_TRY(ev.elapsed(2, 3, &g_times[4]));
    ANR_TRY(ev.elapsed(0, 3, &g_times[5]));
  }
  const unsigned char *O = out.data() - o_kept;
  const int *nk = reinterpret_cast<const int *>(O + o_nk);
  for (int64_t q = 0; q < nq; ++q) {
    if (kept) memcpy(kept + offs[q], O + o_kept + (size_t)offs[q] * 4, (size_t)nk[q] * 4);
    if (n_kept) n_kept[q] = nk[q];
  }
  return ANR_OK;
}

}  // namespace

extern "C" int anr_khop_timing(int32_t enable, float *ms6) {
  g_timing = enable != 0;
  if (ms6) std::copy(g_times, g_times + 6, ms6);
  return ANR_OK;
}

extern "C" int anr_index_khop_rerank(anr_index *h, int32_t device, int64_t nq, const int64_t *offs, const int64_t *rows_host,
                                     const float *query_host, const float *focus_host, const uint8_t *has_focus,
                                     const double *dense_host, const double *focused_host, const double *bm25,
                                     const uint8_t *is_prf, const double *prf_sim, const double *cov, const int32_t *cons,
                                     const int32_t *hop_no, const double *decay, const anr_khop_params *p, double *dense,
                                     double *focused, double *final_score, int32_t *order) {
  const char *what = "khop_rerank";
  if (!h && !dense_host) return fail(ANR_EINVAL, "khop_rerank: null handle without dense scores");
  if (nq < 0) return fail(ANR_EINVAL, "khop_rerank: nq must be >= 0");
  if (nq == 0) return ANR_OK;
  if (!offs || !p) return fail(ANR_EINVAL, "khop_rerank: null offs or parameters");
  const double weights[7] = {p->dense_w, p->bm25_w, p->focused_w2, p->cov_w, p->cons_w, p->rrf_lambda, p->rrf_k};
  ANR_TRY(check_numbers(what, "weight", weights, 7));
  ANR_TRY(check_offs(what, nq, offs));
  const int64_t total = offs[nq];
  if (total == 0) return ANR_OK;
  if (!bm25 || !is_prf || !prf_sim || !cov || !cons || !hop_no || !decay)
    return fail(ANR_EINVAL, "khop_rerank: null candidate array");
  if (!dense_host && (!rows_host || !query_host)) return fail(ANR_EINVAL, "khop_rerank: null rows or query vectors");
  ANR_TRY(check_numbers(what, "bm25", bm25, total));
  ANR_TRY(check_numbers(what, "prf_sim", prf_sim, total));
  ANR_TRY(check_numbers(what, "cov", cov, total));
  ANR_TRY(check_numbers(what, "decay", decay, total));
  if (dense_host) ANR_TRY(check_numbers(what, "dense", dense_host, total));
  if (dense_host && focused_host) ANR_TRY(check_numbers(what, "focused", focused_host, total));
  RerankArgs r{nq,   offs, rows_host, query_host, focus_host, has_focus, dense_host, focused_host, bm25,        prf_sim, cov,
               decay, is_prf, cons,     hop_no,     *p,         dense,     focused,    final_score,  order};
  if (dense_host) {
    const int dev = h ? index_core(h).device : device;
    DeviceGuard g(dev);
    if (!g.ok) return fail(ANR_EHIP, "hipSetDevice(%d) failed", dev);
    DevBuf<unsigned char> arena;  // of this call only: nothing of the handle is read
    return run_rerank(arena, nullptr, 0, r, nullptr);
  }
  const IndexCore c = index_core(h);
  DeviceGuard g(c.device);
  if (!g.ok) return fail(ANR_EHIP, "hipSetDevice(%d) failed", c.device);
  std::lock_guard<std::mutex> lk(*c.mu);
  const IndexCore cur = index_core(h);  // under the lock: an add may have moved the rows
  ANR_TRY(check_rows(what, rows_host, total, cur.ntotal));
  return run_rerank(index_scratch(h).khop_arena, cur.x32, cur.dim, r, cur.stream);
}

extern "C" int anr_index_cluster_suppress(anr_index *h, int32_t device, int64_t nq, const int64_t *offs,
                                          const int64_t *rows_host, const double *sim_host, const double *score_host,
                                          double thr, int32_t keep_m, int32_t *kept, int32_t *n_kept) {
  const char *what = "cluster_suppress";
  if (!h && !sim_host) return fail(ANR_EINVAL, "cluster_suppress: null handle without a similarity matrix");
  if (nq < 0) return fail(ANR_EINVAL, "cluster_suppress: nq must be >= 0");
  if (nq == 0) return ANR_OK;
  if (!offs) return fail(ANR_EINVAL, "cluster_suppress: null offs");
  if (keep_m < 1) return fail(ANR_EINVAL, "cluster_suppress: keep_m must be >= 1");
  if (is_nan(thr)) return fail(ANR_EINVAL, "cluster_suppress: the threshold must be a number");
  ANR_TRY(check_offs(what, nq, offs));
  const int64_t total = offs[nq];
  if (total == 0) {
    if (n_kept) std::fill(n_kept, n_kept + nq, 0);
    return ANR_OK;
  }
  if (!score_host) return fail(ANR_EINVAL, "cluster_suppress: null scores");
  if (!sim_host && !rows_host) return fail(ANR_EINVAL, "cluster_suppress: null rows");
  ANR_TRY(check_numbers(what, "score", score_host, total));
  if (sim_host) {
    const int dev = h ? index_core(h).device : device;
    DeviceGuard g(dev);
    if (!g.ok) return fail(ANR_EHIP, "hipSetDevice(%d) failed", dev);
    DevBuf<unsigned char> sim, arena;  // of this call only
    return run_suppress(sim, arena, nullptr, 0, nq, offs, nullptr, sim_host, score_host, thr, keep_m, kept, n_kept, nullptr);
  }
  const IndexCore c = index_core(h);
  DeviceGuard g(c.device);
  if (!g.ok) return fail(ANR_EHIP, "hipSetDevice(%d) failed", c.device);
  std::lock_guard<std::mutex> lk(*c.mu);
  const IndexCore cur = index_core(h);
  ANR_TRY(check_rows(what, rows_host, total, cur.ntotal));
  IndexScratch &sc = index_scratch(h);
  return run_suppress(sc.khop_sim, sc.khop_arena, cur.x32, cur.dim, nq, offs, rows_host, nullptr, score_host, thr, keep_m, kept,
                      n_kept, cur.stream);
}
