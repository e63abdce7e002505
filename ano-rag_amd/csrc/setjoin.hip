// Set-overlap join: every pair of rows of a family of integer sets that shares at least min_common items, with the
// overlap, the union size and the shared items — the integers behind RelationExtractor.extract_entity_coexistence_relations
// (graph/relation_extractor.py:418-481) — and the overlap / union of an explicit list of row pairs, the integers behind
// _calculate_note_topic_similarity (:738-767) for the in-group pairs of extract_topic_relations (:543-589).
// No floating point anywhere in this file.  DESIGN.md §5k.
//
// Layout on the device: the rows as a CSR (indptr int64 [n_rows + 1], items int32 [nnz], each row strictly ascending)
// and its transpose, the postings (post_ptr int64 [n_items + 1], post_rows int32 [nnz], each posting ascending), built by
// ONE stable radix sort of the keys item << 32 | row.
//
// k_sj_cooccur, one 256-thread workgroup per row i, run twice (count, then fill after an exclusive scan of the per-row
// counts): a wave per item of the row binary-searches the item's posting for the first row of the pass's range and
// strides the tail over its 64 lanes; every j met is accumulated in an open-addressed table in LDS (key by integer
// compare-and-swap, count by integer add, linear probing).  The entries with count >= min_common are compacted, sorted by j
// with a bitonic network in LDS and written; the order in which the atomics landed is gone after the sort, so the output
// is a function of the input alone.  A thread per kept pair then merges the two ascending rows for the shared items.
//
// Overflow rule: a pass may hold at most 3/4 of the table's slots as distinct keys.  A row whose candidates exceed that is
// redone with its range of j, (i, n_rows), cut into P = 2, 4, 8, ... equal-width passes (postings are ascending, so a pass
// is a binary search for its first row and a stop at its last); a pass no wider than the limit always fits, so the
// doubling ends, and whether a pass fits depends on its set of candidates only — P is the same in every run.  The
// count launch records P per row and the fill launch starts there.  No global memory proportional to the candidates.
//
// Cost: an item present in L rows is walked L^2 / 2 times over all its rows — the size of the reference's own candidate
// set (its `related_notes` unions); documented, not avoided.
#include <algorithm>
#include <mutex>

#include "common.hpp"
#include "setjoin.hpp"

namespace anr {

using u64 = unsigned long long;

struct SjOut {
  int32_t *I, *J, *inter, *uni;
  int64_t *cptr;
  int32_t *citems;
  int64_t n_pairs, n_common;
};

// stats slots the fill launch adds to (integer adds: the sums do not depend on the order)
enum { kSjStRows = 0, kSjStInsert = 1, kSjStOverflowed = 2, kSjStPasses = 3, kSjStBroken = 4, kSjStN = 8 };

// keys item << 32 | row of every CSR entry: the row of entry k is the last r with indptr[r] <= k
__global__ void k_sj_keys(const int64_t *indptr, const int32_t *items, int64_t n_rows, int64_t nnz, u64 *keys) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nnz) return;
  int64_t l = 0, r = n_rows;  // first r in [0, n_rows] with indptr[r] > k, minus one
  while (l < r) {
    const int64_t m = (l + r) >> 1;
    if (indptr[m + 1] <= k) l = m + 1;
    else r = m;
  }
  keys[k] = ((u64)(unsigned)items[k] << 32) | (u64)(unsigned)l;
}

// post_ptr[e] = the first sorted key of item e or above; post_rows = the keys' low halves
__global__ void k_sj_post_ptr(const u64 *sorted, int64_t nnz, int64_t n_items, int64_t *post_ptr) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e > n_items) return;
  const u64 want = (u64)e << 32;
  int64_t l = 0, r = nnz;
  while (l < r) {
    const int64_t m = (l + r) >> 1;
    if (sorted[m] < want) l = m + 1;
    else r = m;
  }
  post_ptr[e] = l;
}
__global__ void k_sj_post_rows(const u64 *sorted, int64_t nnz, int32_t *post_rows) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < nnz) post_rows[k] = (int32_t)(unsigned)(sorted[k] & 0xffffffffull);
}

// exclusive prefix sum of in[0..n) into out[0..n], out[n] = the total (one workgroup, a carry across 1024-entry chunks)
__global__ __launch_bounds__(1024) void k_sj_scan(const int64_t *in, int64_t n, int64_t *out) {
  __shared__ int64_t wsum[16];
  __shared__ int64_t carry_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int64_t c0 = 0; c0 < n; c0 += 1024) {
    const int64_t i = c0 + tid;
    const int64_t x = i < n ? in[i] : 0;
    int64_t incl = x;
    for (int o = 1; o < 64; o <<= 1) {
      const int64_t t = __shfl_up(incl, o);
      if (lane >= o) incl += t;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int64_t off = carry_s;
    for (int w = 0; w < wave; ++w) off += wsum[w];
    if (i < n) out[i] = off + incl - x;
    __syncthreads();
    if (tid == 1023) carry_s = off + incl;
    __syncthreads();
  }
  if (tid == 0) out[n] = carry_s;
}

// FILL = false: row_pairs[i], row_common[i], row_passes[i] <- the pairs kept, the shared items and the passes of row i.
// FILL = true: pair_off / common_off are the exclusive scans of the first two; the pairs of row i go to
// [pair_off[i], pair_off[i + 1]) ascending by j, their shared items to common_off[i] onwards in the same order.
template <bool FILL>
__global__ __launch_bounds__(kSjThreads) void k_sj_cooccur(int64_t n_rows, const int64_t *__restrict__ indptr,
                                                           const int32_t *__restrict__ items,
                                                           const int64_t *__restrict__ post_ptr,
                                                           const int32_t *__restrict__ post_rows, unsigned min_common,
                                                           int S, int log_s, int64_t *row_pairs, int64_t *row_common,
                                                           int32_t *row_passes, const int64_t *pair_off,
                                                           const int64_t *common_off, SjOut o, u64 *stats) {
  extern __shared__ __align__(16) unsigned char sj_lds[];
  u64 *outb = reinterpret_cast<u64 *>(sj_lds);           // [S] compacted (j << 32 | count), then sorted
  int *keys = reinterpret_cast<int *>(outb + S);         // [S] table keys, -1 = free; after the sort: shared-item offsets
  unsigned *cnts = reinterpret_cast<unsigned *>(keys + S);  // [S] table counts
  unsigned *part = cnts + S;                             // [kSjThreads] per-thread sums of the shared-item prefix
  u64 &s_ins = *reinterpret_cast<u64 *>(part + kSjThreads), &s_shared = *(&s_ins + 1);
  unsigned *s_u = reinterpret_cast<unsigned *>(&s_ins + 2);
  unsigned &s_distinct = s_u[0], &s_flag = s_u[1], &s_kept = s_u[2];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t i = blockIdx.x;
  if (i >= n_rows) return;
  const int64_t a0 = indptr[i], a1 = indptr[i + 1], len_i = a1 - a0;
  const int64_t span = n_rows - 1 - i;  // the candidate rows are i + 1 .. n_rows - 1
  if (len_i == 0 || span <= 0) {
    if (!FILL && tid == 0) {
      row_pairs[i] = 0;
      row_common[i] = 0;
      row_passes[i] = 0;
    }
    return;
  }
  const unsigned cap = (unsigned)sj_table_fill(S);
  int64_t P = FILL ? (int64_t)row_passes[i] : 1;
  int64_t npairs = 0, ncommon = 0;
  u64 ins = 0;
  for (;;) {
    const int64_t W = (span + P - 1) / P;
    bool ok = true;
    npairs = 0;
    ncommon = 0;
    ins = 0;
    for (int64_t p = 0; p < P && ok; ++p) {
      const int64_t lo = i + 1 + p * W;
      if (lo >= n_rows) break;
      const int64_t hi = lo + W < n_rows ? lo + W : n_rows;
      for (int s = tid; s < S; s += kSjThreads) {
        keys[s] = -1;
        cnts[s] = 0u;
      }
      if (tid == 0) {
        s_distinct = 0u;
        s_flag = 0u;
        s_kept = 0u;
        s_ins = 0ull;
        s_shared = 0ull;
      }
      __syncthreads();
      // ---- accumulate: a wave per item, the posting's tail inside [lo, hi) over the lanes
      u64 my_ins = 0;
      for (int64_t t = a0 + wave; t < a1; t += kSjThreads / 64) {
        const int32_t e = items[t];
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
          unsigned h = ((unsigned)j * 2654435761u) >> (32 - log_s);
          bool done = false;
          for (int probe = 0; probe < S; ++probe) {
            const int prev = atomicCAS(&keys[h], -1, j);
            if (prev == -1 && atomicAdd(&s_distinct, 1u) + 1u > cap) atomicExch(&s_flag, 1u);
            if (prev == -1 || prev == j) {
              atomicAdd(&cnts[h], 1u);
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
        u64 sh = 0;
        for (int s = tid; s < S; s += kSjThreads)
          if (keys[s] != -1 && cnts[s] >= min_common) {
            ++k;
            sh += cnts[s];
          }
        if (k) {
          atomicAdd(&s_kept, k);
          atomicAdd(&s_shared, sh);
        }
        __syncthreads();
        npairs += s_kept;
        ncommon += (int64_t)s_shared;
        ins += s_ins;
        __syncthreads();
        continue;
      }
      // ---- compact the kept entries (any order), pad to a power of two, sort ascending by j
      for (int s = tid; s < S; s += kSjThreads)
        if (keys[s] != -1 && cnts[s] >= min_common) {
          const unsigned pos = atomicAdd(&s_kept, 1u);
          outb[pos] = ((u64)(unsigned)keys[s] << 32) | (u64)cnts[s];
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
              const u64 a = outb[t], b = outb[x];
              if ((a > b) == ((t & k2) == 0)) {
                outb[t] = b;
                outb[x] = a;
              }
            }
          }
          __syncthreads();
        }
      // ---- where each pair's shared items go: an exclusive prefix of the counts, a contiguous chunk per thread
      const int chunk = (K + kSjThreads - 1) / kSjThreads;
      const int c0 = tid * chunk < K ? tid * chunk : K, c1 = c0 + chunk < K ? c0 + chunk : K;
      unsigned mine = 0;
      for (int t = c0; t < c1; ++t) mine += (unsigned)(outb[t] & 0xffffffffull);
      part[tid] = mine;
      __syncthreads();  // also: every read of the table's keys is done, the array is reused below
      unsigned pre = 0, total = 0;
      for (int t = 0; t < kSjThreads; ++t) {
        if (t == tid) pre = total;
        total += part[t];
      }
      for (int t = c0; t < c1; ++t) {
        keys[t] = (int)pre;
        pre += (unsigned)(outb[t] & 0xffffffffull);
      }
      __syncthreads();
      const int64_t pbase = pair_off[i] + npairs, cbase = common_off[i] + ncommon;
      for (int k = tid; k < K; k += kSjThreads) {
        const u64 v = outb[k];
        const int j = (int)(unsigned)(v >> 32);
        const unsigned c = (unsigned)(v & 0xffffffffull);
        const int64_t g = pbase + k;
        if (g >= o.n_pairs) continue;  // cannot happen: the count launch sized the output from the same tables
        const int64_t b0 = indptr[j], b1 = indptr[j + 1];
        o.I[g] = (int32_t)i;
        o.J[g] = j;
        o.inter[g] = (int32_t)c;
        o.uni[g] = (int32_t)(len_i + (b1 - b0) - (int64_t)c);
        const int64_t dst = cbase + (int64_t)(unsigned)keys[k];
        o.cptr[g] = dst;
        int64_t a = a0, b = b0;
        unsigned w = 0;
        while (a < a1 && b < b1 && w < c) {  // both rows ascending
          const int32_t x = items[a], y = items[b];
          if (x == y && dst + w < o.n_common) o.citems[dst + w] = x;
          w += x == y;
          a += x <= y;
          b += y <= x;
        }
      }
      npairs += K;
      ncommon += total;
      ins += s_ins;
      __syncthreads();
    }
    if (ok) break;
    if (FILL) {  // cannot happen: the count launch found P passes to fit
      if (tid == 0) atomicAdd(&stats[kSjStBroken], 1ull);
      return;
    }
    P *= 2;
  }
  if (tid == 0) {
    if (!FILL) {
      row_pairs[i] = npairs;
      row_common[i] = ncommon;
      row_passes[i] = (int32_t)P;
    } else {
      atomicAdd(&stats[kSjStRows], 1ull);
      atomicAdd(&stats[kSjStInsert], ins);
      atomicAdd(&stats[kSjStPasses], (u64)P);
      if (P > 1) atomicAdd(&stats[kSjStOverflowed], 1ull);
    }
  }
}

// overlap and union size of n explicit row pairs: kSjPairLanes lanes per pair.  The longer list is cut into one contiguous
// chunk per lane; a lane finds its chunk's start in the other list by binary search and merges from there with a
// branch-light two-pointer step; the group's counts are added with shuffles and lane 0 stores.
__global__ __launch_bounds__(256) void k_sj_pair_counts(int64_t n, const int32_t *__restrict__ I, const int32_t *__restrict__ J,
                                                        const int64_t *__restrict__ indptr, const int32_t *__restrict__ items,
                                                        int32_t *inter, int32_t *uni) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t pair = gid / kSjPairLanes;
  const int sub = (int)(gid % kSjPairLanes);
  const bool valid = pair < n;
  int cnt = 0;
  int64_t la = 0, lb = 0;
  if (valid) {
    const int32_t *A = items + indptr[I[pair]], *B = items + indptr[J[pair]];
    la = indptr[I[pair] + 1] - indptr[I[pair]];
    lb = indptr[J[pair] + 1] - indptr[J[pair]];
    if (la < lb) {
      const int32_t *tp = A; A = B; B = tp;
      const int64_t tl = la; la = lb; lb = tl;
    }
    const int64_t chunk = (la + kSjPairLanes - 1) / kSjPairLanes;
    const int64_t s = sub * chunk < la ? sub * chunk : la, e = s + chunk < la ? s + chunk : la;
    if (s < e && lb > 0) {
      const int32_t first = A[s];
      int64_t l = 0, r = lb;
      while (l < r) {
        const int64_t m = (l + r) >> 1;
        if (B[m] < first) l = m + 1;
        else r = m;
      }
      int64_t a = s, b = l;
      while (a < e && b < lb) {
        const int32_t x = A[a], y = B[b];
        cnt += x == y;
        a += x <= y;
        b += y <= x;
      }
    }
  }
  for (int off = kSjPairLanes / 2; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
  if (valid && sub == 0) {
    inter[pair] = cnt;
    uni[pair] = (int32_t)(la + lb - cnt);
  }
}

}  // namespace anr

using namespace anr;

struct anr_setjoin {
  int device = 0;
  int64_t n_rows = 0, n_items = 0, nnz = 0;
  DevBuf<int64_t> indptr, post_ptr;
  DevBuf<int32_t> items, post_rows;
  hipStream_t stream = nullptr;
  std::mutex mu;
  int slots = kSjDefaultSlots;
  // the result of the last anr_setjoin_cooccur
  bool has_result = false;
  int64_t n_pairs = 0, n_common = 0;
  DevBuf<int32_t> rI, rJ, rInter, rUni, rItems;
  DevBuf<int64_t> rPtr;
};

namespace {

inline unsigned sj_blocks(int64_t n, int per = 256) { return (unsigned)std::max<int64_t>(1, ceil_div(n, per)); }

void free_result(anr_setjoin *h) {
  for (auto *b : {&h->rI, &h->rJ, &h->rInter, &h->rUni, &h->rItems}) b->release();
  h->rPtr.release();
  h->has_result = false;
  h->n_pairs = h->n_common = 0;
}

}  // namespace

extern "C" {

int anr_setjoin_create(int64_t n_rows, int64_t n_items, const int64_t *indptr, const int32_t *items, int32_t device,
                       anr_setjoin **out) {
  if (!out) return fail(ANR_EINVAL, "out is null");
  *out = nullptr;
  if (n_rows < 0 || n_rows >= 0x7fffffffll) return fail(ANR_EINVAL, "n_rows must be in [0, 2^31 - 1)");
  if (n_items < 0 || n_items >= 0x7fffffffll) return fail(ANR_EINVAL, "n_items must be in [0, 2^31 - 1)");
  if (!indptr) return fail(ANR_EINVAL, "indptr is null");
  if (indptr[0] != 0) return fail(ANR_EINVAL, "indptr[0] must be 0");
  for (int64_t r = 0; r < n_rows; ++r) {
    const int64_t len = indptr[r + 1] - indptr[r];
    if (len < 0) return fail(ANR_EINVAL, "indptr descends at row %lld", (long long)r);
    if (len > kSjMaxRowLen) return fail(ANR_EINVAL, "row %lld has %lld items, at most %lld", (long long)r, (long long)len, (long long)kSjMaxRowLen);
  }
  const int64_t nnz = indptr[n_rows];
  if (nnz >= 0x7fffffffll) return fail(ANR_EINVAL, "at most 2^31 - 2 entries");
  if (nnz > 0 && !items) return fail(ANR_EINVAL, "items is null");
  for (int64_t r = 0; r < n_rows; ++r)
    for (int64_t k = indptr[r]; k < indptr[r + 1]; ++k) {
      if (items[k] < 0 || items[k] >= n_items)
        return fail(ANR_EINVAL, "row %lld: item id %d outside [0, %lld)", (long long)r, items[k], (long long)n_items);
      if (k > indptr[r] && items[k] <= items[k - 1])
        return fail(ANR_EINVAL, "row %lld: item ids must be strictly ascending (%d after %d)", (long long)r, items[k], items[k - 1]);
    }
  int ndev = anr_device_count();
  if (ndev <= 0) return fail(ANR_EHIP, "no HIP device is visible");
  if (device < 0 || device >= ndev) return fail(ANR_EINVAL, "device %d out of range", device);
  DeviceGuard g(device);
  anr_setjoin *h = new anr_setjoin();
  h->device = device;
  h->n_rows = n_rows;
  h->n_items = n_items;
  h->nnz = nnz;
  auto body = [&]() -> int {  // a failure destroys the handle below
    DevBuf<u64> k0, k1;         // the sort's buffers, of this call only
    DevBuf<unsigned> v0, v1;
    DevBuf<unsigned char> temp;
    ANR_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    hipStream_t st = h->stream;
    ANR_TRY(h->indptr.alloc(n_rows + 1, "setjoin"));
    ANR_TRY(h->items.alloc(nnz, "setjoin"));
    ANR_TRY(h->post_ptr.alloc(n_items + 1, "setjoin"));
    ANR_TRY(h->post_rows.alloc(nnz, "setjoin"));
    ANR_HIP(hipMemcpyAsync(h->indptr.p, indptr, (size_t)(n_rows + 1) * 8, hipMemcpyHostToDevice, st));
    if (nnz > 0) {
      ANR_HIP(hipMemcpyAsync(h->items.p, items, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
      ANR_TRY(k0.alloc(nnz, "setjoin"));
      ANR_TRY(k1.alloc(nnz, "setjoin"));
      ANR_TRY(v0.alloc(nnz, "setjoin"));
      ANR_TRY(v1.alloc(nnz, "setjoin"));
      ANR_TRY(temp.alloc((int64_t)radix_sort_temp_bytes(nnz), "setjoin"));
      ANR_HIP(hipMemsetAsync(v0.p, 0, (size_t)nnz * 4, st));  // the sort carries a value per key; the keys are all there is
      hipLaunchKernelGGL(k_sj_keys, dim3(sj_blocks(nnz)), dim3(256), 0, st, h->indptr.p, h->items.p, n_rows, nnz, k0.p);
      ANR_TRY(radix_sort_pairs_u64(temp.p, k0.p, k1.p, v0.p, v1.p, nnz, false, st));
      hipLaunchKernelGGL(k_sj_post_rows, dim3(sj_blocks(nnz)), dim3(256), 0, st, k1.p, nnz, h->post_rows.p);
    }
    hipLaunchKernelGGL(k_sj_post_ptr, dim3(sj_blocks(n_items + 1)), dim3(256), 0, st, k1.p, nnz, n_items, h->post_ptr.p);
    ANR_HIP(hipGetLastError());
    ANR_HIP(hipStreamSynchronize(st));
    return ANR_OK;
  };
  const int rc = body();
  if (rc != ANR_OK) {
    anr_setjoin_destroy(h);
    return rc;
  }
  *out = h;
  return ANR_OK;
}

int anr_setjoin_destroy(anr_setjoin *h) {
  if (!h) return ANR_OK;
  DeviceGuard g(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  free_result(h);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;  // frees the rows and the postings, still under the guard
  return ANR_OK;
}

int anr_setjoin_set_option(anr_setjoin *h, int32_t option, int64_t value) {
  if (!h) return fail(ANR_EINVAL, "null handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (option == ANR_SETJOIN_OPT_TABLE_SLOTS) {
    if (value == 0) value = kSjDefaultSlots;
    if (value < kSjMinSlots || value > kSjMaxSlots || (value & (value - 1)))
      return fail(ANR_EINVAL, "table slots must be a power of two in [%d, %d] (0 = the default, %d)", kSjMinSlots, kSjMaxSlots,
                  kSjDefaultSlots);
    h->slots = (int)value;
    return ANR_OK;
  }
  return fail(ANR_EINVAL, "unknown setjoin option %d", option);
}

int anr_setjoin_cooccur(anr_setjoin *h, int32_t min_common, int64_t *n_pairs, int64_t *n_common, int64_t *stats8) {
  if (!h) return fail(ANR_EINVAL, "null handle");
  if (min_common < 1) return fail(ANR_EINVAL, "min_common must be at least 1");
  std::lock_guard<std::mutex> lk(h->mu);
  DeviceGuard g(h->device);
  hipStream_t st = h->stream;
  free_result(h);
  const int64_t n = h->n_rows;
  const int S = h->slots;
  int log_s = 0;
  while ((1 << log_s) < S) ++log_s;
  const int lds = sj_lds_bytes(S);
  u64 hs[kSjStN] = {0};
  int64_t tot[2] = {0, 0};
  const int64_t scratch = n > 0 && h->nnz > 0 ? (n * 2 + (n + 1) * 2) * 8 + n * 4 + kSjStN * 8 : 0;
  auto body = [&]() -> int {  // a failure frees the partial result below
    if (n == 0 || h->nnz == 0) return ANR_OK;
    DevBuf<int64_t> row_pairs, row_common, pair_off, common_off;  // scratch of this call
    DevBuf<int32_t> row_passes;
    DevBuf<u64> d_stats;
    ANR_TRY(row_pairs.alloc(n, "setjoin"));
    ANR_TRY(row_common.alloc(n, "setjoin"));
    ANR_TRY(row_passes.alloc(n, "setjoin"));
    ANR_TRY(pair_off.alloc(n + 1, "setjoin"));
    ANR_TRY(common_off.alloc(n + 1, "setjoin"));
    ANR_TRY(d_stats.alloc(kSjStN, "setjoin"));
    ANR_HIP(hipMemsetAsync(d_stats.p, 0, kSjStN * 8, st));
    ANR_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(&k_sj_cooccur<false>), sj_lds_bytes(kSjMaxSlots)));
    ANR_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(&k_sj_cooccur<true>), sj_lds_bytes(kSjMaxSlots)));
    SjOut none{};
    hipLaunchKernelGGL((k_sj_cooccur<false>), dim3((unsigned)n), dim3(kSjThreads), lds, st, n, h->indptr.p, h->items.p,
                       h->post_ptr.p, h->post_rows.p, (unsigned)min_common, S, log_s, row_pairs.p, row_common.p, row_passes.p,
                       nullptr, nullptr, none, d_stats.p);
    hipLaunchKernelGGL(k_sj_scan, dim3(1), dim3(1024), 0, st, row_pairs.p, n, pair_off.p);
    hipLaunchKernelGGL(k_sj_scan, dim3(1), dim3(1024), 0, st, row_common.p, n, common_off.p);
    ANR_HIP(hipGetLastError());
    ANR_HIP(hipMemcpyAsync(&tot[0], pair_off.p + n, 8, hipMemcpyDeviceToHost, st));
    ANR_HIP(hipMemcpyAsync(&tot[1], common_off.p + n, 8, hipMemcpyDeviceToHost, st));
    ANR_HIP(hipStreamSynchronize(st));
    // the output: 16 bytes + an offset per pair, 4 bytes per shared item — an error when it does not fit, never a cut
    const int64_t need = tot[0] * 24 + 8 + tot[1] * 4;
    size_t free_b = 0, total_b = 0;
    ANR_HIP(hipMemGetInfo(&free_b, &total_b));
    if ((u64)need > (u64)free_b)
      return fail(ANR_EHIP, "co-occurrence result does not fit: %lld pairs and %lld shared items need %lld bytes, %lld are free "
                  "on the device; raise min_common", (long long)tot[0], (long long)tot[1], (long long)need, (long long)free_b);
    ANR_TRY(h->rI.alloc(tot[0], "setjoin"));
    ANR_TRY(h->rJ.alloc(tot[0], "setjoin"));
    ANR_TRY(h->rInter.alloc(tot[0], "setjoin"));
    ANR_TRY(h->rUni.alloc(tot[0], "setjoin"));
    ANR_TRY(h->rPtr.alloc(tot[0] + 1, "setjoin"));
    ANR_TRY(h->rItems.alloc(tot[1], "setjoin"));
    SjOut o{h->rI.p, h->rJ.p, h->rInter.p, h->rUni.p, h->rPtr.p, h->rItems.p, tot[0], tot[1]};
    hipLaunchKernelGGL((k_sj_cooccur<true>), dim3((unsigned)n), dim3(kSjThreads), lds, st, n, h->indptr.p, h->items.p,
                       h->post_ptr.p, h->post_rows.p, (unsigned)min_common, S, log_s, row_pairs.p, row_common.p, row_passes.p,
                       pair_off.p, common_off.p, o, d_stats.p);
    ANR_HIP(hipGetLastError());
    ANR_HIP(hipMemcpyAsync(h->rPtr.p + tot[0], &tot[1], 8, hipMemcpyHostToDevice, st));
    ANR_HIP(hipMemcpyAsync(hs, d_stats.p, kSjStN * 8, hipMemcpyDeviceToHost, st));
    ANR_HIP(hipStreamSynchronize(st));
    if (hs[kSjStBroken]) return fail(ANR_EINTERNAL, "co-occurrence: the fill launch disagreed with the count launch on %llu rows", hs[kSjStBroken]);
    return ANR_OK;
  };
  const int rc = body();
  if (rc != ANR_OK) {
    free_result(h);
    return rc;
  }
  h->has_result = true;
  h->n_pairs = tot[0];
  h->n_common = tot[1];
  if (n_pairs) *n_pairs = tot[0];
  if (n_common) *n_common = tot[1];
  if (stats8) {
    stats8[0] = (int64_t)hs[kSjStRows];
    stats8[1] = (int64_t)hs[kSjStInsert];
    stats8[2] = tot[0];
    stats8[3] = tot[1];
    stats8[4] = (int64_t)hs[kSjStOverflowed];
    stats8[5] = S;
    stats8[6] = (int64_t)hs[kSjStPasses];
    stats8[7] = scratch;
  }
  return ANR_OK;
}

int anr_setjoin_cooccur_fetch(anr_setjoin *h, int32_t *I, int32_t *J, int32_t *inter, int32_t *uni, int64_t *common_ptr,
                              int32_t *common_items) {
  if (!h) return fail(ANR_EINVAL, "null handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->has_result) return fail(ANR_ESTATE, "anr_setjoin_cooccur_fetch before anr_setjoin_cooccur");
  if (!common_ptr) return fail(ANR_EINVAL, "common_ptr is null");
  const int64_t np = h->n_pairs, nc = h->n_common;
  if (np == 0) {
    common_ptr[0] = 0;
    return ANR_OK;
  }
  if (!I || !J || !inter || !uni || (nc > 0 && !common_items)) return fail(ANR_EINVAL, "null output array");
  DeviceGuard g(h->device);
  hipStream_t st = h->stream;
  ANR_HIP(hipMemcpyAsync(I, h->rI.p, (size_t)np * 4, hipMemcpyDeviceToHost, st));
  ANR_HIP(hipMemcpyAsync(J, h->rJ.p, (size_t)np * 4, hipMemcpyDeviceToHost, st));
  ANR_HIP(hipMemcpyAsync(inter, h->rInter.p, (size_t)np * 4, hipMemcpyDeviceToHost, st));
  ANR_HIP(hipMemcpyAsync(uni, h->rUni.p, (size_t)np * 4, hipMemcpyDeviceToHost, st));
  ANR_HIP(hipMemcpyAsync(common_ptr, h->rPtr.p, (size_t)(np + 1) * 8, hipMemcpyDeviceToHost, st));
  if (nc > 0) ANR_HIP(hipMemcpyAsync(common_items, h->rItems.p, (size_t)nc * 4, hipMemcpyDeviceToHost, st));
  ANR_HIP(hipStreamSynchronize(st));
  return ANR_OK;
}

int anr_setjoin_pair_counts(anr_setjoin *h, int64_t n, const int32_t *I, const int32_t *J, int32_t *inter, int32_t *uni) {
  if (!h) return fail(ANR_EINVAL, "null handle");
  if (n < 0 || n > (1ll << 40) / kSjPairLanes) return fail(ANR_EINVAL, "bad pair count");
  if (n == 0) return ANR_OK;
  if (!I || !J || !inter || !uni) return fail(ANR_EINVAL, "null pair array");
  for (int64_t k = 0; k < n; ++k)
    if (I[k] < 0 || I[k] >= h->n_rows || J[k] < 0 || J[k] >= h->n_rows)
      return fail(ANR_EINVAL, "pair %lld: row outside [0, %lld)", (long long)k, (long long)h->n_rows);
  std::lock_guard<std::mutex> lk(h->mu);
  DeviceGuard g(h->device);
  hipStream_t st = h->stream;
  DevBuf<int32_t> dI, dJ, dA, dU;  // of this call
  ANR_TRY(dI.alloc(n, "setjoin"));
  ANR_TRY(dJ.alloc(n, "setjoin"));
  ANR_TRY(dA.alloc(n, "setjoin"));
  ANR_TRY(dU.alloc(n, "setjoin"));
  ANR_HIP(hipMemcpyAsync(dI.p, I, (size_t)n * 4, hipMemcpyHostToDevice, st));
  ANR_HIP(hipMemcpyAsync(dJ.p, J, (size_t)n * 4, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_sj_pair_counts, dim3(sj_blocks(n * kSjPairLanes)), dim3(256), 0, st, n, dI.p, dJ.p, h->indptr.p,
                     h->items.p, dA.p, dU.p);
  ANR_HIP(hipGetLastError());
  ANR_HIP(hipMemcpyAsync(inter, dA.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  ANR_HIP(hipMemcpyAsync(uni, dU.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  ANR_HIP(hipStreamSynchronize(st));
  return ANR_OK;
}

}  // extern "C"
