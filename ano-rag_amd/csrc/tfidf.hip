// TF-IDF cosine join and search: every pair of rows of a sparse float64 matrix whose dot product reaches a threshold — the
// pairs NoteValidator._find_semantic_duplicates (utils/note_validator.py:363-393) reads out of the dense N x N
// cosine_similarity matrix — and the per-document sums of VectorRetriever._bm25_search (vector_store/retriever.py:966-1002).
// Compiled with -ffp-contract=off: every value is `s = s + a * b`, one rounded multiply and one rounded add, in ascending
// label order — scipy's own order once the terms carry the labels of anorag_hip.note_dedup.relabel_terms.  DESIGN.md §5o
// has the order argument, the layout, the proof of the nominating bound and the cost.
//
// Device layout: the CSR (indptr, terms, vals; rows strictly ascending in label) and the postings (post_ptr, post_rows,
// post_vals; ascending in row) from ONE stable radix sort of term << 32 | row that carries the entry's position; the key,
// posting and scan kernels are setjoin.hip's own.
//
// Stage one, k_tf_nominate (the shape of k_sj_cooccur, same table, overflow rule and count-then-fill launches): candidate
// j of row i accumulates N = sum ceil(a * b * 2^30) by INTEGER LDS add — independent of the order of the atomics, and
// 2^30 * s < N + 1/4 for the float sum s decided later, so N >= floor(2^30 * threshold) nominates every pair that passes;
// N < 2^30 + 2^11 + 2^20 by the unit-row check of create.
// Stage two, k_tf_decide: 8 lanes per nominated pair find the shared terms in parallel and add the products ONE AT A TIME
// in ascending label; k_tf_compact writes the pairs with s >= threshold in (i, j) order around a scan.  No floating-point
// atomics, no output cursor.  Stage one costs L^2 / 2 insertions for a term present in L rows; documented, not avoided.
// k_tf_scores: a workgroup per query, terms in the order given, a barrier between terms; a document occurs once in a
// posting, so its value is 0.0 + w_0 * m + w_1 * m + ... in the query's order.
#include <algorithm>
#include <cmath>
#include <mutex>

#include "common.hpp"
#include "setjoin.hpp"

namespace anr {

using u64 = unsigned long long;

constexpr int kTfPairLanes = 8;          // lanes that share one pair of k_tf_decide
constexpr double kTfScale = 1073741824.0;  // 2^30: the fixed point of the nominating bound
constexpr double kTfUnitSlack = 1.0 / 1048576.0;  // a row's sum of squares may exceed 1 by 2^-20

// stats slots the fill launch adds to (integer adds: the sums do not depend on the order)
enum { kTfStRows = 0, kTfStInsert = 1, kTfStOverflowed = 2, kTfStBroken = 3, kTfStN = 4 };

__global__ void k_tf_iota(int64_t n, unsigned *v) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) v[k] = (unsigned)k;
}

// post_vals[k] = the value of the CSR entry the k-th sorted key came from
__global__ void k_tf_post_vals(const unsigned *perm, const double *vals, int64_t nnz, double *post_vals) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < nnz) post_vals[k] = vals[perm[k]];
}

// FILL = false: row_pairs[i], row_passes[i] <- the pairs row i nominates and the passes it needed.
// FILL = true: pair_off is the exclusive scan of row_pairs; the pairs of row i go to [pair_off[i], pair_off[i + 1])
// ascending by j.
template <bool FILL>
__global__ __launch_bounds__(kSjThreads) void k_tf_nominate(int64_t n_rows, const int64_t *__restrict__ indptr,
                                                            const int32_t *__restrict__ terms,
                                                            const double *__restrict__ vals,
                                                            const int64_t *__restrict__ post_ptr,
                                                            const int32_t *__restrict__ post_rows,
                                                            const double *__restrict__ post_vals, unsigned thr_fx, int S,
                                                            int log_s, int64_t *row_pairs, int32_t *row_passes,
                                                            const int64_t *pair_off, int32_t *nomI, int32_t *nomJ,
                                                            int64_t n_nom, u64 *stats) {
  extern __shared__ __align__(16) unsigned char tf_lds[];
  u64 *outb = reinterpret_cast<u64 *>(tf_lds);              // [S] compacted (j << 32 | sum), then sorted
  int *keys = reinterpret_cast<int *>(outb + S);            // [S] table keys, -1 = free
  unsigned *sums = reinterpret_cast<unsigned *>(keys + S);  // [S] table sums of ceil(a * b * 2^30)
  u64 &s_ins = *reinterpret_cast<u64 *>(sums + S);
  unsigned *s_u = reinterpret_cast<unsigned *>(&s_ins + 1);
  unsigned &s_distinct = s_u[0], &s_flag = s_u[1], &s_kept = s_u[2];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t i = blockIdx.x;
  if (i >= n_rows) return;
  const int64_t a0 = indptr[i], a1 = indptr[i + 1];
  const int64_t span = n_rows - 1 - i;  // the candidate rows are i + 1 .. n_rows - 1
  if (a1 == a0 || span <= 0) {
    if (!FILL && tid == 0) {
      row_pairs[i] = 0;
      row_passes[i] = 0;
    }
    return;
  }
  const unsigned cap = (unsigned)sj_table_fill(S);
  int64_t P = FILL ? (int64_t)row_passes[i] : 1;
  int64_t npairs = 0;
  u64 ins = 0;
  for (;;) {
    const int64_t W = (span + P - 1) / P;
    bool ok = true;
    npairs = 0;
    ins = 0;
    for (int64_t p = 0; p < P && ok; ++p) {
      const int64_t lo = i + 1 + p * W;
      if (lo >= n_rows) break;
      const int64_t hi = lo + W < n_rows ? lo + W : n_rows;
      for (int s = tid; s < S; s += kSjThreads) {
        keys[s] = -1;
        sums[s] = 0u;
      }
      if (tid == 0) {
        s_distinct = 0u;
        s_flag = 0u;
        s_kept = 0u;
        s_ins = 0ull;
      }
      __syncthreads();
      // ---- accumulate: a wave per term, the posting's tail inside [lo, hi) over the lanes
      u64 my_ins = 0;
      for (int64_t t = a0 + wave; t < a1; t += kSjThreads / 64) {
        const int32_t e = terms[t];
        const double a = vals[t];
        const int64_t q1 = post_ptr[e + 1];
        int64_t l = post_ptr[e], r = q1;
        while (l < r) {  // the first entry of the posting with row >= lo
          const int64_t m = (l + r) >> 1;
          if (post_rows[m] < lo) l = m + 1;
          else r = m;
        }
        for (int64_t q = l + lane; q < q1; q += 64) {
          const int j = post_rows[q];
          if (j >= hi) break;
          if (*reinterpret_cast<volatile unsigned *>(&s_flag)) break;  // the pass is abandoned already
          const unsigned add = (unsigned)ceil((a * post_vals[q]) * kTfScale);  // <= 2^30 + 2^11 by the unit-row check
          unsigned h = ((unsigned)j * 2654435761u) >> (32 - log_s);
          bool done = false;
          for (int probe = 0; probe < S; ++probe) {
            const int prev = atomicCAS(&keys[h], -1, j);
            if (prev == -1 && atomicAdd(&s_distinct, 1u) + 1u > cap) atomicExch(&s_flag, 1u);
            if (prev == -1 || prev == j) {
              atomicAdd(&sums[h], add);
              done = true;
              break;
            }
            h = (h + 1u) & (unsigned)(S - 1);
          }
          if (!done) atomicExch(&s_flag, 1u);
          ++my_ins;
        }
      }
      if (my_ins) atomicAdd(&s_ins, my_ins);
      __syncthreads();
      const bool overflow = s_flag != 0u;
      if (overflow) {
        ok = false;
        __syncthreads();  // everyone has read s_flag before the next pass resets it
        break;
      }
      if (!FILL) {
        unsigned k = 0;
        for (int s = tid; s < S; s += kSjThreads) k += keys[s] != -1 && sums[s] >= thr_fx;
        if (k) atomicAdd(&s_kept, k);
        __syncthreads();
        npairs += s_kept;
        ins += s_ins;
        __syncthreads();
        continue;
      }
      // ---- compact the nominated entries (any order), pad to a power of two, sort ascending by j
      for (int s = tid; s < S; s += kSjThreads)
        if (keys[s] != -1 && sums[s] >= thr_fx) {
          const unsigned pos = atomicAdd(&s_kept, 1u);
          outb[pos] = ((u64)(unsigned)keys[s] << 32) | (u64)sums[s];
        }
      __syncthreads();
      const int K = (int)s_kept;  // <= cap < S
      int M = 1;
      while (M < K) M <<= 1;      // <= S
      for (int t = K + tid; t < M; t += kSjThreads) outb[t] = ~0ull;
      __syncthreads();
      for (int k2 = 2; k2 <= M; k2 <<= 1)
        for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
          for (int t = tid; t < M; t += kSjThreads) {
            const int x = t ^ j2;
            if (x > t) {
              const u64 va = outb[t], vb = outb[x];
              if ((va > vb) == ((t & k2) == 0)) {
                outb[t] = vb;
                outb[x] = va;
              }
            }
          }
          __syncthreads();
        }
      const int64_t pbase = pair_off[i] + npairs;
      for (int k = tid; k < K; k += kSjThreads) {
        const int64_t g = pbase + k;
        if (g >= n_nom) continue;  // cannot happen: the count launch sized the output from the same tables
        nomI[g] = (int32_t)i;
        nomJ[g] = (int32_t)(unsigned)(outb[k] >> 32);
      }
      npairs += K;
      ins += s_ins;
      __syncthreads();
    }
    if (ok) break;
    if (FILL) {  // cannot happen: the count launch found P passes to fit
      if (tid == 0) atomicAdd(&stats[kTfStBroken], 1ull);
      return;
    }
    P *= 2;
  }
  if (tid == 0) {
    if (!FILL) {
      row_pairs[i] = npairs;
      row_passes[i] = (int32_t)P;
    } else {
      atomicAdd(&stats[kTfStRows], 1ull);
      atomicAdd(&stats[kTfStInsert], ins);
      if (P > 1) atomicAdd(&stats[kTfStOverflowed], 1ull);
    }
  }
}

// the exact value of n nominated pairs: kTfPairLanes lanes per pair (all lanes of a group run the same trips)
__global__ __launch_bounds__(256) void k_tf_decide(int64_t n, const int32_t *__restrict__ I, const int32_t *__restrict__ J,
                                                   const int64_t *__restrict__ indptr, const int32_t *__restrict__ terms,
                                                   const double *__restrict__ vals, double *sim) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t pair = gid / kTfPairLanes;
  const int sub = (int)(gid % kTfPairLanes);
  const bool valid = pair < n;
  const int32_t *A = terms, *B = terms;
  const double *VA = vals, *VB = vals;
  int64_t la = 0, lb = 0;
  if (valid) {
    const int64_t i0 = indptr[I[pair]], j0 = indptr[J[pair]];
    la = indptr[I[pair] + 1] - i0;
    lb = indptr[J[pair] + 1] - j0;
    A = terms + i0, VA = vals + i0;
    B = terms + j0, VB = vals + j0;
    if (la > lb) {  // walk the shorter row; the order of the additions is ascending label either way
      const int32_t *tp = A; A = B; B = tp;
      const double *tv = VA; VA = VB; VB = tv;
      const int64_t tl = la; la = lb; lb = tl;
    }
  }
  double s = 0.0;
  int64_t lo = 0;  // nothing of B below lo can match what is left of A
  for (int64_t base = 0; base < la; base += kTfPairLanes) {
    const int64_t a = base + sub;
    double p = 0.0;
    int64_t l = lb;
    if (a < la) {
      const int32_t x = A[a];
      int64_t r = lb;
      l = lo;
      while (l < r) {
        const int64_t m = (l + r) >> 1;
        if (B[m] < x) l = m + 1;
        else r = m;
      }
      if (l < lb && B[l] == x) p = VA[a] * VB[l];
    }
    for (int k = 0; k < kTfPairLanes; ++k) s = s + __shfl(p, k, kTfPairLanes);
    lo = __shfl(l, kTfPairLanes - 1, kTfPairLanes);
  }
  if (valid && sub == 0) sim[pair] = s;
}

// a wave per row.  FILL = false: row_kept[i] <- the nominated pairs of row i with sim >= threshold.  FILL = true: they go
// to [kept_off[i], kept_off[i + 1]) in their order, which is ascending j.
template <bool FILL>
__global__ __launch_bounds__(256) void k_tf_compact(int64_t n_rows, const int64_t *__restrict__ nom_off,
                                                    const int32_t *__restrict__ nomJ, const double *__restrict__ sim,
                                                    double threshold, int64_t *row_kept, const int64_t *kept_off,
                                                    int32_t *outI, int32_t *outJ, double *out_sim, int64_t n_kept) {
  const int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (row >= n_rows) return;
  const int64_t b0 = nom_off[row], b1 = nom_off[row + 1];
  int64_t cnt = 0;
  for (int64_t q = b0; q < b1; q += 64) {
    const int64_t k = q + lane;
    const bool keep = k < b1 && sim[k] >= threshold;
    const u64 m = __ballot(keep);
    if (FILL && keep) {
      const int64_t pos = kept_off[row] + cnt + __popcll(m & ((1ull << lane) - 1ull));
      if (pos < n_kept) {  // cannot fail: the count launch read the same values
        outI[pos] = (int32_t)row;
        outJ[pos] = nomJ[k];
        out_sim[pos] = sim[k];
      }
    }
    cnt += __popcll(m);
  }
  if (!FILL && lane == 0) row_kept[row] = cnt;
}

// out[q][d] = 0.0 + w_0 * m_d + w_1 * m_d + ... over the terms of query q in the order given (out arrives zeroed)
__global__ __launch_bounds__(256) void k_tf_scores(const int64_t *__restrict__ q_indptr, const int32_t *__restrict__ q_terms,
                                                   const double *__restrict__ q_w, const int64_t *__restrict__ post_ptr,
                                                   const int32_t *__restrict__ post_rows,
                                                   const double *__restrict__ post_vals, int64_t n_rows, double *out) {
  const int64_t q = blockIdx.x;
  double *o = out + q * n_rows;
  for (int64_t t = q_indptr[q]; t < q_indptr[q + 1]; ++t) {  // the same trips for the whole workgroup
    const int32_t e = q_terms[t];
    const double w = q_w[t];
    for (int64_t p = post_ptr[e] + threadIdx.x; p < post_ptr[e + 1]; p += blockDim.x) {
      const int32_t d = post_rows[p];
      o[d] = o[d] + w * post_vals[p];
    }
    __syncthreads();  // the next term's update of a document follows this one's
  }
}

}  // namespace anr

using namespace anr;

struct anr_tfidf {
  int device = 0;
  int64_t n_rows = 0, n_terms = 0, nnz = 0;
  DevBuf<int64_t> indptr, post_ptr;
  DevBuf<int32_t> terms, post_rows;
  DevBuf<double> vals, post_vals;
  hipStream_t stream = nullptr;
  std::mutex mu;
  int slots = kSjDefaultSlots;
  // the result of the last anr_tfidf_self_join
  bool has_result = false;
  int64_t n_pairs = 0;
  DevBuf<int32_t> rI, rJ;
  DevBuf<double> rSim;
};

namespace {

inline unsigned tf_blocks(int64_t n, int per = 256) { return (unsigned)std::max<int64_t>(1, ceil_div(n, per)); }

void free_result(anr_tfidf *h) {
  h->rI.release();
  h->rJ.release();
  h->rSim.release();
  h->has_result = false;
  h->n_pairs = 0;
}

}  // namespace

extern "C" {

int anr_tfidf_create(int32_t device, int64_t n_rows, int64_t n_terms, const int64_t *indptr, const int32_t *terms,
                     const double *values, anr_tfidf **out) {
  if (!out) return fail(ANR_EINVAL, "out is null");
  *out = nullptr;
  if (n_rows < 0 || n_rows >= 0x7fffffffll) return fail(ANR_EINVAL, "n_rows must be in [0, 2^31 - 1)");
  if (n_terms < 0 || n_terms >= 0x7fffffffll) return fail(ANR_EINVAL, "n_terms must be in [0, 2^31 - 1)");
  if (!indptr) return fail(ANR_EINVAL, "indptr is null");
  if (indptr[0] != 0) return fail(ANR_EINVAL, "indptr[0] must be 0");
  for (int64_t r = 0; r < n_rows; ++r) {
    const int64_t len = indptr[r + 1] - indptr[r];
    if (len < 0) return fail(ANR_EINVAL, "indptr descends at row %lld", (long long)r);
    if (len > kSjMaxRowLen) return fail(ANR_EINVAL, "row %lld has %lld terms, at most %lld", (long long)r, (long long)len, (long long)kSjMaxRowLen);
  }
  const int64_t nnz = indptr[n_rows];
  if (nnz >= 0x7fffffffll) return fail(ANR_EINVAL, "at most 2^31 - 2 entries");
  if (nnz > 0 && (!terms || !values)) return fail(ANR_EINVAL, "terms or values is null");
  for (int64_t r = 0; r < n_rows; ++r) {
    double sq = 0.0;
    for (int64_t k = indptr[r]; k < indptr[r + 1]; ++k) {
      if (terms[k] < 0 || terms[k] >= n_terms)
        return fail(ANR_EINVAL, "row %lld: term label %d outside [0, %lld)", (long long)r, terms[k], (long long)n_terms);
      if (k > indptr[r] && terms[k] <= terms[k - 1])
        return fail(ANR_EINVAL, "row %lld: term labels must be strictly ascending (%d after %d)", (long long)r, terms[k], terms[k - 1]);
      if (!std::isfinite(values[k]) || values[k] < 0.0)
        return fail(ANR_EINVAL, "row %lld: value %g is not a finite number >= 0", (long long)r, values[k]);
      sq += values[k] * values[k];
    }
    if (!(sq <= 1.0 + kTfUnitSlack))
      return fail(ANR_EINVAL, "row %lld: sum of squares %.17g exceeds 1 + 2^-20; pass rows of unit length", (long long)r, sq);
  }
  int ndev = anr_device_count();
  if (ndev <= 0) return fail(ANR_EHIP, "no HIP device is visible");
  if (device < 0 || device >= ndev) return fail(ANR_EINVAL, "device %d out of range", device);
  DeviceGuard g(device);
  anr_tfidf *h = new anr_tfidf();
  h->device = device;
  h->n_rows = n_rows;
  h->n_terms = n_terms;
  h->nnz = nnz;
  auto body = [&]() -> int {  // a failure destroys the handle below
    DevBuf<u64> k0, k1;         // the sort's buffers, of this call only
    DevBuf<unsigned> v0, v1;
    DevBuf<unsigned char> temp;
    ANR_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    hipStream_t st = h->stream;
    ANR_TRY(h->indptr.alloc(n_rows + 1, "tfidf"));
    ANR_TRY(h->terms.alloc(nnz, "tfidf"));
    ANR_TRY(h->vals.alloc(nnz, "tfidf"));
    ANR_TRY(h->post_ptr.alloc(n_terms + 1, "tfidf"));
    ANR_TRY(h->post_rows.alloc(nnz, "tfidf"));
    ANR_TRY(h->post_vals.alloc(nnz, "tfidf"));
    ANR_HIP(hipMemcpyAsync(h->indptr.p, indptr, (size_t)(n_rows + 1) * 8, hipMemcpyHostToDevice, st));
    if (nnz > 0) {
      ANR_HIP(hipMemcpyAsync(h->terms.p, terms, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
      ANR_HIP(hipMemcpyAsync(h->vals.p, values, (size_t)nnz * 8, hipMemcpyHostToDevice, st));
      ANR_TRY(k0.alloc(nnz, "tfidf"));
      ANR_TRY(k1.alloc(nnz, "tfidf"));
      ANR_TRY(v0.alloc(nnz, "tfidf"));
      ANR_TRY(v1.alloc(nnz, "tfidf"));
      ANR_TRY(temp.alloc((int64_t)radix_sort_temp_bytes(nnz), "tfidf"));
      hipLaunchKernelGGL(k_tf_iota, dim3(tf_blocks(nnz)), dim3(256), 0, st, nnz, v0.p);  // the sort carries each entry's position
      hipLaunchKernelGGL(k_sj_keys, dim3(tf_blocks(nnz)), dim3(256), 0, st, h->indptr.p, h->terms.p, n_rows, nnz, k0.p);
      ANR_TRY(radix_sort_pairs_u64(temp.p, k0.p, k1.p, v0.p, v1.p, nnz, false, st));
      hipLaunchKernelGGL(k_sj_post_rows, dim3(tf_blocks(nnz)), dim3(256), 0, st, k1.p, nnz, h->post_rows.p);
      hipLaunchKernelGGL(k_tf_post_vals, dim3(tf_blocks(nnz)), dim3(256), 0, st, v1.p, h->vals.p, nnz, h->post_vals.p);
    }
    hipLaunchKernelGGL(k_sj_post_ptr, dim3(tf_blocks(n_terms + 1)), dim3(256), 0, st, k1.p, nnz, n_terms, h->post_ptr.p);
    ANR_HIP(hipGetLastError());
    ANR_HIP(hipStreamSynchronize(st));
    return ANR_OK;
  };
  const int rc = body();
  if (rc != ANR_OK) {
    anr_tfidf_destroy(h);
    return rc;
  }
  *out = h;
  return ANR_OK;
}

int anr_tfidf_destroy(anr_tfidf *h) {
  if (!h) return ANR_OK;
  DeviceGuard g(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  free_result(h);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;  // frees the rows and the postings, still under the guard
  return ANR_OK;
}

int anr_tfidf_set_option(anr_tfidf *h, int32_t option, int64_t value) {
  if (!h) return fail(ANR_EINVAL, "null handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (option == ANR_TFIDF_OPT_TABLE_SLOTS) {
    if (value == 0) value = kSjDefaultSlots;
    if (value < kSjMinSlots || value > kSjMaxSlots || (value & (value - 1)))
      return fail(ANR_EINVAL, "table slots must be a power of two in [%d, %d] (0 = the default, %d)", kSjMinSlots, kSjMaxSlots,
                  kSjDefaultSlots);
    h->slots = (int)value;
    return ANR_OK;
  }
  return fail(ANR_EINVAL, "unknown tfidf option %d", option);
}

int anr_tfidf_self_join(anr_tfidf *h, double threshold, int64_t *n_pairs, int64_t *stats8) {
  if (!h) return fail(ANR_EINVAL, "null handle");
  if (!(threshold > 0.0) || threshold > 2.0)
    return fail(ANR_EINVAL, "threshold must be in (0, 2]: a pair that shares no term is never looked at");
  std::lock_guard<std::mutex> lk(h->mu);
  DeviceGuard g(h->device);
  hipStream_t st = h->stream;
  free_result(h);
  const int64_t n = h->n_rows;
  const int S = h->slots;
  int log_s = 0;
  while ((1 << log_s) < S) ++log_s;
  const int lds = sj_lds_bytes(S);
  const unsigned thr_fx = (unsigned)std::floor(threshold * kTfScale);  // <= 2^31
  u64 hs[kTfStN] = {0};
  int64_t n_nom = 0, n_kept = 0;
  float ms_nom = 0.f, ms_dec = 0.f;
  auto body = [&]() -> int {  // a failure frees the partial result below
    if (n == 0 || h->nnz == 0) return ANR_OK;
    DevBuf<int64_t> row_cnt, off;  // scratch of this call: per-row counts and their scan, used by both stages in turn
    DevBuf<int32_t> row_passes, nomI, nomJ;
    DevBuf<double> sim;
    DevBuf<u64> d_stats;
    Events<3> ev;
    ANR_TRY(ev.init());
    ANR_TRY(row_cnt.alloc(n, "tfidf"));
    ANR_TRY(off.alloc(n + 1, "tfidf"));
    ANR_TRY(row_passes.alloc(n, "tfidf"));
    ANR_TRY(d_stats.alloc(kTfStN, "tfidf"));
    ANR_HIP(hipMemsetAsync(d_stats.p, 0, kTfStN * 8, st));
    ANR_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(&k_tf_nominate<false>), sj_lds_bytes(kSjMaxSlots)));
    ANR_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(&k_tf_nominate<true>), sj_lds_bytes(kSjMaxSlots)));
    ANR_TRY(ev.mark(0, st));
    hipLaunchKernelGGL((k_tf_nominate<false>), dim3((unsigned)n), dim3(kSjThreads), lds, st, n, h->indptr.p, h->terms.p,
                       h->vals.p, h->post_ptr.p, h->post_rows.p, h->post_vals.p, thr_fx, S, log_s, row_cnt.p, row_passes.p,
                       nullptr, nullptr, nullptr, (int64_t)0, d_stats.p);
    hipLaunchKernelGGL(k_sj_scan, dim3(1), dim3(1024), 0, st, row_cnt.p, n, off.p);
    ANR_HIP(hipGetLastError());
    ANR_HIP(hipMemcpyAsync(&n_nom, off.p + n, 8, hipMemcpyDeviceToHost, st));
    ANR_HIP(hipStreamSynchronize(st));
    // 16 bytes a nominated pair, 16 more a kept one — an error when they do not fit, never a cut
    size_t free_b = 0, total_b = 0;
    ANR_HIP(hipMemGetInfo(&free_b, &total_b));
    if ((u64)n_nom * 32ull > (u64)free_b)
      return fail(ANR_EHIP, "self join: %lld nominated pairs need %lld bytes, %lld are free on the device; raise the threshold",
                  (long long)n_nom, (long long)(n_nom * 32), (long long)free_b);
    ANR_TRY(nomI.alloc(n_nom, "tfidf"));
    ANR_TRY(nomJ.alloc(n_nom, "tfidf"));
    ANR_TRY(sim.alloc(n_nom, "tfidf"));
    hipLaunchKernelGGL((k_tf_nominate<true>), dim3((unsigned)n), dim3(kSjThreads), lds, st, n, h->indptr.p, h->terms.p,
                       h->vals.p, h->post_ptr.p, h->post_rows.p, h->post_vals.p, thr_fx, S, log_s, row_cnt.p, row_passes.p,
                       off.p, nomI.p, nomJ.p, n_nom, d_stats.p);
    ANR_TRY(ev.mark(1, st));
    if (n_nom > 0)
      hipLaunchKernelGGL(k_tf_decide, dim3(tf_blocks(n_nom * kTfPairLanes)), dim3(256), 0, st, n_nom, nomI.p, nomJ.p,
                         h->indptr.p, h->terms.p, h->vals.p, sim.p);
    // off is still the scan of the nominated counts: keep it as nom_off, scan the kept counts into a second buffer
    DevBuf<int64_t> kept_off;
    ANR_TRY(kept_off.alloc(n + 1, "tfidf"));
    hipLaunchKernelGGL((k_tf_compact<false>), dim3(tf_blocks(n * 64)), dim3(256), 0, st, n, off.p, nomJ.p, sim.p, threshold,
                       row_cnt.p, nullptr, nullptr, nullptr, nullptr, (int64_t)0);
    hipLaunchKernelGGL(k_sj_scan, dim3(1), dim3(1024), 0, st, row_cnt.p, n, kept_off.p);
    ANR_HIP(hipGetLastError());
    ANR_HIP(hipMemcpyAsync(&n_kept, kept_off.p + n, 8, hipMemcpyDeviceToHost, st));
    ANR_HIP(hipStreamSynchronize(st));
    ANR_TRY(h->rI.alloc(n_kept, "tfidf"));
    ANR_TRY(h->rJ.alloc(n_kept, "tfidf"));
    ANR_TRY(h->rSim.alloc(n_kept, "tfidf"));
    hipLaunchKernelGGL((k_tf_compact<true>), dim3(tf_blocks(n * 64)), dim3(256), 0, st, n, off.p, nomJ.p, sim.p, threshold,
                       row_cnt.p, kept_off.p, h->rI.p, h->rJ.p, h->rSim.p, n_kept);
    ANR_TRY(ev.mark(2, st));
    ANR_HIP(hipGetLastError());
    ANR_HIP(hipMemcpyAsync(hs, d_stats.p, kTfStN * 8, hipMemcpyDeviceToHost, st));
    ANR_HIP(hipStreamSynchronize(st));
    ANR_TRY(ev.elapsed(0, 1, &ms_nom));
    ANR_TRY(ev.elapsed(1, 2, &ms_dec));
    if (hs[kTfStBroken]) return fail(ANR_EINTERNAL, "self join: the fill launch disagreed with the count launch on %llu rows", hs[kTfStBroken]);
    return ANR_OK;
  };
  const int rc = body();
  if (rc != ANR_OK) {
    free_result(h);
    return rc;
  }
  h->has_result = true;
  h->n_pairs = n_kept;
  if (n_pairs) *n_pairs = n_kept;
  if (stats8) {
    stats8[0] = (int64_t)hs[kTfStRows];
    stats8[1] = (int64_t)hs[kTfStInsert];
    stats8[2] = n_nom;
    stats8[3] = n_kept;
    stats8[4] = (int64_t)hs[kTfStOverflowed];
    stats8[5] = S;
    stats8[6] = (int64_t)(ms_nom * 1000.0f);
    stats8[7] = (int64_t)(ms_dec * 1000.0f);
  }
  return ANR_OK;
}

int anr_tfidf_self_join_fetch(anr_tfidf *h, int32_t *I, int32_t *J, double *sim) {
  if (!h) return fail(ANR_EINVAL, "null handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->has_result) return fail(ANR_ESTATE, "anr_tfidf_self_join_fetch before anr_tfidf_self_join");
  const int64_t np = h->n_pairs;
  if (np == 0) return ANR_OK;
  if (!I || !J || !sim) return fail(ANR_EINVAL, "null output array");
  DeviceGuard g(h->device);
  hipStream_t st = h->stream;
  ANR_HIP(hipMemcpyAsync(I, h->rI.p, (size_t)np * 4, hipMemcpyDeviceToHost, st));
  ANR_HIP(hipMemcpyAsync(J, h->rJ.p, (size_t)np * 4, hipMemcpyDeviceToHost, st));
  ANR_HIP(hipMemcpyAsync(sim, h->rSim.p, (size_t)np * 8, hipMemcpyDeviceToHost, st));
  ANR_HIP(hipStreamSynchronize(st));
  return ANR_OK;
}

int anr_tfidf_scores(anr_tfidf *h, int64_t nq, const int64_t *q_indptr, const int32_t *q_terms, const double *q_weights,
                     double *out_host) {
  if (!h) return fail(ANR_EINVAL, "null handle");
  if (nq < 0 || nq >= 0x7fffffffll) return fail(ANR_EINVAL, "nq must be in [0, 2^31 - 1)");
  if (nq == 0) return ANR_OK;
  if (!q_indptr) return fail(ANR_EINVAL, "q_indptr is null");
  if (q_indptr[0] != 0) return fail(ANR_EINVAL, "q_indptr[0] must be 0");
  for (int64_t q = 0; q < nq; ++q)
    if (q_indptr[q + 1] < q_indptr[q]) return fail(ANR_EINVAL, "q_indptr descends at query %lld", (long long)q);
  const int64_t qnnz = q_indptr[nq];
  if (qnnz >= 0x7fffffffll) return fail(ANR_EINVAL, "at most 2^31 - 2 query terms");
  if (qnnz > 0 && (!q_terms || !q_weights)) return fail(ANR_EINVAL, "q_terms or q_weights is null");
  for (int64_t k = 0; k < qnnz; ++k) {
    if (q_terms[k] < 0 || q_terms[k] >= h->n_terms)
      return fail(ANR_EINVAL, "query term label %d outside [0, %lld)", q_terms[k], (long long)h->n_terms);
    if (!std::isfinite(q_weights[k])) return fail(ANR_EINVAL, "query weight %lld is not finite", (long long)k);
  }
  if (h->n_rows == 0) return ANR_OK;
  if (nq > (1ll << 37) / h->n_rows) return fail(ANR_EINVAL, "nq * n_rows must be at most 2^37 values; cut the batch");
  if (!out_host) return fail(ANR_EINVAL, "out_host is null");
  std::lock_guard<std::mutex> lk(h->mu);
  DeviceGuard g(h->device);
  hipStream_t st = h->stream;
  const int64_t n_out = nq * h->n_rows;
  DevBuf<int64_t> d_ptr;  // of this call
  DevBuf<int32_t> d_terms;
  DevBuf<double> d_w, d_out;
  ANR_TRY(d_ptr.alloc(nq + 1, "tfidf"));
  ANR_TRY(d_terms.alloc(qnnz, "tfidf"));
  ANR_TRY(d_w.alloc(qnnz, "tfidf"));
  ANR_TRY(d_out.alloc(n_out, "tfidf", 0, "the scores"));
  ANR_HIP(hipMemcpyAsync(d_ptr.p, q_indptr, (size_t)(nq + 1) * 8, hipMemcpyHostToDevice, st));
  if (qnnz > 0) {
    ANR_HIP(hipMemcpyAsync(d_terms.p, q_terms, (size_t)qnnz * 4, hipMemcpyHostToDevice, st));
    ANR_HIP(hipMemcpyAsync(d_w.p, q_weights, (size_t)qnnz * 8, hipMemcpyHostToDevice, st));
  }
  ANR_HIP(hipMemsetAsync(d_out.p, 0, (size_t)n_out * 8, st));  // all bits zero is +0.0
  hipLaunchKernelGGL(k_tf_scores, dim3((unsigned)nq), dim3(256), 0, st, d_ptr.p, d_terms.p, d_w.p, h->post_ptr.p,
                     h->post_rows.p, h->post_vals.p, h->n_rows, d_out.p);
  ANR_HIP(hipGetLastError());
  ANR_HIP(hipMemcpyAsync(out_host, d_out.p, (size_t)n_out * 8, hipMemcpyDeviceToHost, st));
  ANR_HIP(hipStreamSynchronize(st));
  return ANR_OK;
}

}  // extern "C"
