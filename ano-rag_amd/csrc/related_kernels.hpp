// Device kernels of anr_index_related_notes (related.hip): NoteSimilarityCalculator.find_related_notes
// (utils/note_similarity.py:115-233) over the stored rows of a cosine index.  Three steps per strip of rows:
// the MFMA tile walk of the self join (join_tile_mma, join_tile.hpp) nominates the pairs whose f16 score can still pass,
// an 8-lane group per pair scores it from the float32 rows and the sorted entity rows, and one wave per row selects the
// first M of its kept pairs.  No floating-point atomics; nothing depends on the order in which pairs were appended.
#pragma once
#include "common.hpp"
#include "join_tile.hpp"
#include "setjoin.hpp"

namespace anr {

// counters of one strip, device side
enum { kRelCand = 0, kRelBand = 1, kRelRecords = 2, kRelCounters = 4 };

struct RelatedWalk {
  const uint4 *x16;
  int kb;
  int64_t n_rows, n_tiles;
  PatchGrid pg;        // (block rows of the strip) x (all blocks)
  int64_t n_slots;
  int bi0;             // first 256-row block of the strip
  int row_lo, row_hi;  // the strip: pairs (i, j), i < j, with row_lo <= i < row_hi
  // f16 score >= thr_lo: nominated; of those, score <= thr_hi: the image alone could not tell (counted, not treated apart)
  float thr_lo, thr_hi;
  const int *cluster;  // [n_rows] codes, -1 = none
  int exclude_same;    // drop pairs with c_i == c_j != -1 here
  uint2 *cand;
  unsigned long long cap;
  unsigned long long *counters;
};

// One walk of the block pairs (bi, bj >= bi) of a strip of block rows; the diagonal block computes both orders of its
// pairs and keeps i < j.  Emission is the DBSCAN degree walk's: one reservation per wave, nothing written past the cap
// (the host reads the count and cuts the strip if it was passed).
__global__ __launch_bounds__(512) void k_related_walk(RelatedWalk p) {
  constexpr int TM = 8, TN = 8;
  extern __shared__ uint4 lds[];  // join_tile_mma's 128 KiB
  __shared__ __attribute__((aligned(16))) int s_c[512];  // cluster codes of the tile pair's rows, i rows then j rows
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n_rows = (int)p.n_rows;
  for (int64_t slot = blockIdx.x; slot < p.n_slots; slot += gridDim.x) {
    int bi, bj;
    if (!patch_tile(p.pg, slot, bi, bj)) continue;
    bi += p.bi0;
    if (bi > bj) continue;
    const int64_t tb0 = (int64_t)bi * TM, nb0 = (int64_t)bj * TN;
    const int wm = wave >> 1, wn = wave & 1;
    {
      const int t = threadIdx.x;
      const int row = t < 256 ? (int)tb0 * 32 + t : (int)nb0 * 32 + t - 256;
      s_c[t] = (p.exclude_same && row < n_rows) ? p.cluster[row] : -1;  // visible after the barriers of the product
    }
    floatx16 acc[2][4];
    join_tile_mma(p.x16, p.kb, p.n_tiles, tb0, nb0, lds, lane, wave, acc);

    unsigned em[2][4];
    unsigned nem = 0, nband = 0;
    int ci[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) ci[m] = s_c[(2 * wm + m) * 32 + (lane & 31)];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int lj0 = (4 * wn + n) * 32 + 4 * (lane >> 5);
      int cj[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int4 v = *reinterpret_cast<const int4 *>(&s_c[256 + lj0 + 8 * q]);
        cj[4 * q] = v.x; cj[4 * q + 1] = v.y; cj[4 * q + 2] = v.z; cj[4 * q + 3] = v.w;
      }
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const int gi = (int)(tb0 + 2 * wm + m) * 32 + (lane & 31);
        const int gj0 = (int)nb0 * 32 + lj0;
        const bool irow = gi >= p.row_lo && gi < p.row_hi;
        unsigned e = 0, b = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int gj = gj0 + (r & 3) + 8 * (r >> 2);
          const float s = acc[m][n][r];
          const bool ok = irow && gi < gj && gj < n_rows && !(ci[m] == cj[r] && cj[r] != -1) && s >= p.thr_lo;
          e |= ok ? (1u << r) : 0u;
          b |= (ok && !(s > p.thr_hi)) ? (1u << r) : 0u;
        }
        em[m][n] = e;
        nem += (unsigned)__popc(e);
        nband += (unsigned)__popc(b);
        __builtin_amdgcn_sched_barrier(0);  // one fragment's 64 comparisons at a time: hoisted together they spill scalar registers
      }
    }
    if (__ballot(nem != 0u) != 0ull) {
      unsigned incl = nem, bsum = nband;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const unsigned v = __shfl_up(incl, off), w = __shfl_up(bsum, off);
        if (lane >= off) incl += v, bsum += w;
      }
      unsigned long long base = 0;
      if (lane == 63) {
        base = atomicAdd(p.counters + kRelCand, (unsigned long long)incl);
        if (bsum) atomicAdd(p.counters + kRelBand, (unsigned long long)bsum);
      }
      unsigned long long k = __shfl(base, 63) + (incl - nem);
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          const unsigned gi = (unsigned)((tb0 + 2 * wm + m) * 32 + (lane & 31));
          const unsigned gj0 = (unsigned)((nb0 + 4 * wn + n) * 32 + 4 * (lane >> 5));
          unsigned h = em[m][n];
          while (h) {
            const int r = __ffs(h) - 1;
            h &= h - 1;
            if (k < p.cap) p.cand[k] = make_uint2(gi, gj0 + (r & 3) + 8 * (r >> 2));
            ++k;
          }
        }
    }
    __syncthreads();  // s_c is rewritten by the next tile pair
  }
}

struct RelatedScore {
  const float *x32;
  int dim;
  const uint2 *cand;
  unsigned long long n_cand;
  const int *cluster;
  const int64_t *indptr;
  const int32_t *ids;
  double threshold, thr_bonus /* threshold - 0.1 */, one_minus_w, w, bonus;
  int min_shared, exclude_same;
  // directed records of the kept pairs, two per pair: 2 * n_cand of each
  unsigned long long *rec_row;  // sort key
  unsigned *rec_idx;            // sort value: the record's own index
  int *rec_col, *rec_inter, *rec_uni;
  double *rec_comb, *rec_base;
  unsigned long long *counters;
};

// |A & B| of two strictly ascending rows by the kSjPairLanes lanes of a group (the merge of k_sj_pair_counts, setjoin.hip):
// the longer row is cut into one chunk per lane, a lane finds its chunk's start in the other row by binary search
__device__ __forceinline__ int related_overlap(const int32_t *A, int64_t la, const int32_t *B, int64_t lb, int sub) {
  if (la < lb) {
    const int32_t *tp = A; A = B; B = tp;
    const int64_t tl = la; la = lb; lb = tl;
  }
  int cnt = 0;
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
  return cnt;
}

// One group of kSjPairLanes = 8 lanes per nominated pair.  base: lane l adds the exact products of k = l, l + 8, ... in
// ascending k, the eight sums are joined by the xor butterfly 4, 2, 1 — ((0+4)+(2+6)) + ((1+5)+(3+7)) on every lane; the
// file is compiled without contraction.
__global__ __launch_bounds__(256) void k_related_score(RelatedScore p) {
  const int lane = threadIdx.x & 63, sub = lane & (kSjPairLanes - 1);
  const unsigned long long per_block = 256 / kSjPairLanes;
  for (unsigned long long c0 = (unsigned long long)blockIdx.x * per_block; c0 < p.n_cand;
       c0 += (unsigned long long)gridDim.x * per_block) {
    const unsigned long long c = c0 + threadIdx.x / kSjPairLanes;
    const bool valid = c < p.n_cand;
    const uint2 e = valid ? p.cand[c] : make_uint2(0u, 0u);
    const float *a = p.x32 + (int64_t)e.x * p.dim, *b = p.x32 + (int64_t)e.y * p.dim;
    double base = 0.0;
    if (valid)
      for (int k = sub; k < p.dim; k += kSjPairLanes) base += (double)a[k] * (double)b[k];
    int inter = 0;
    int64_t la = 0, lb = 0;
    if (valid) {
      const int64_t a0 = p.indptr[e.x], b0 = p.indptr[e.y];
      la = p.indptr[e.x + 1] - a0;
      lb = p.indptr[e.y + 1] - b0;
      inter = related_overlap(p.ids + a0, la, p.ids + b0, lb, sub);
    }
#pragma unroll
    for (int off = kSjPairLanes / 2; off > 0; off >>= 1) {
      base += __shfl_xor(base, off);
      inter += __shfl_xor(inter, off);
    }
    const int uni = (int)(la + lb) - inter;
    double ent;
    if (la == 0 && lb == 0) ent = 0.5;
    else if (la == 0 || lb == 0) ent = 0.0;
    else {
      ent = (double)inter / (double)uni;
      if (inter >= p.min_shared) ent += 0.1;
      ent = ent < 1.0 ? ent : 1.0;
    }
    double cb = 0.0;
    if (valid && !p.exclude_same && p.cluster[e.x] != p.cluster[e.y] && base > p.thr_bonus) cb = p.bonus;
    const double combined = base * p.one_minus_w + ent * p.w + cb;
    const bool keep = valid && sub == 0 && combined > p.threshold;
    const unsigned long long mask = __ballot(keep);
    if (mask) {
      unsigned long long at = 0;
      const int first = __ffsll((long long)mask) - 1;
      if (lane == first) at = atomicAdd(p.counters + kRelRecords, 2ull * (unsigned long long)__popcll(mask));
      at = __shfl(at, first);
      if (keep) {
        const unsigned long long r = at + 2ull * (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));  // 2 per pair: it fits
        p.rec_row[r] = e.x;      p.rec_row[r + 1] = e.y;
        p.rec_idx[r] = (unsigned)r; p.rec_idx[r + 1] = (unsigned)(r + 1);
        p.rec_col[r] = (int)e.y; p.rec_col[r + 1] = (int)e.x;
        p.rec_comb[r] = combined; p.rec_comb[r + 1] = combined;
        p.rec_base[r] = base;    p.rec_base[r + 1] = base;
        p.rec_inter[r] = inter;  p.rec_inter[r + 1] = inter;
        p.rec_uni[r] = uni;      p.rec_uni[r + 1] = uni;
      }
    }
  }
}

struct RelatedSelect {
  int64_t n_rows;
  int M;
  // the strip's records sorted by row
  const unsigned long long *key;  // [n_rec] rows ascending
  const unsigned *val;            // [n_rec] record indices
  unsigned long long n_rec;
  unsigned *seg_lo, *seg_hi;      // [n_rows] the row's segment of key / val (both 0: none)
  const int *rec_col, *rec_inter, *rec_uni;
  const double *rec_comb, *rec_base;
  // per-row top M kept so far, also the call's result
  int *nbr, *n_nbr, *inter, *uni;
  double *comb, *base;
};

__global__ __launch_bounds__(256) void k_related_segments(RelatedSelect p) {
  const unsigned long long k = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= p.n_rec) return;
  const unsigned long long row = p.key[k];
  if (k == 0 || p.key[k - 1] != row) p.seg_lo[row] = (unsigned)k;
  if (k + 1 == p.n_rec || p.key[k + 1] != row) p.seg_hi[row] = (unsigned)(k + 1);
}

// a comes before b in a row's result: combined descending, then column ascending
__device__ __forceinline__ bool related_before(double ca, int ja, double cb, int jb) {
  return ca > cb || (ca == cb && ja < jb);
}

// One wave per row: the first M of (the row's kept entries of earlier strips) + (its records of this strip), by M rounds
// of "the best entry that comes after the last one taken".  The order is total (a column appears once in a row), so the
// result is a function of the set of entries alone.
__global__ __launch_bounds__(256) void k_related_select(RelatedSelect p) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.n_rows) return;
  const unsigned lo = p.seg_lo[row], hi = p.seg_hi[row];
  if (lo == hi) return;  // nothing new for this row
  const int M = p.M;
  const int64_t o = row * M;
  const int n_old = p.n_nbr[row];
  // the entries kept so far wait in registers, one per lane (M <= 64), while the slots are rewritten
  const bool has_old = lane < n_old;
  const double oc = has_old ? p.comb[o + lane] : 0.0, ob = has_old ? p.base[o + lane] : 0.0;
  const int oj = has_old ? p.nbr[o + lane] : -1, oi = has_old ? p.inter[o + lane] : 0, ou = has_old ? p.uni[o + lane] : 0;
  double last_c = __builtin_huge_val();
  int last_j = -1;
  int t = 0;
  for (; t < M; ++t) {
    // src: < 0 none; bit 30 set: the old entry of lane (src & 63); else position in val
    double bc = 0.0;
    int bjn = 0, src = -1;
    if (has_old && related_before(last_c, last_j, oc, oj)) bc = oc, bjn = oj, src = (1 << 30) | lane;
    for (unsigned k = lo + lane; k < hi; k += 64) {
      const unsigned r = p.val[k];
      const double c = p.rec_comb[r];
      const int j = p.rec_col[r];
      if (related_before(last_c, last_j, c, j) && (src < 0 || related_before(c, j, bc, bjn))) bc = c, bjn = j, src = (int)(k - lo);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double c2 = __shfl_xor(bc, off);
      const int j2 = __shfl_xor(bjn, off), s2 = __shfl_xor(src, off);
      if (s2 >= 0 && (src < 0 || related_before(c2, j2, bc, bjn))) bc = c2, bjn = j2, src = s2;
    }
    if (src < 0) break;  // uniform: every lane holds the same winner
    const bool from_old = (src >> 30) & 1;
    const int ol = src & 63;
    const double wb_old = __shfl(ob, ol);
    const int wi_old = __shfl(oi, ol), wu_old = __shfl(ou, ol);
    if (lane == 0) {
      double wb = wb_old;
      int wi = wi_old, wu = wu_old;
      if (!from_old) {
        const unsigned r = p.val[lo + (unsigned)src];
        wb = p.rec_base[r], wi = p.rec_inter[r], wu = p.rec_uni[r];
      }
      p.nbr[o + t] = bjn;
      p.comb[o + t] = bc;
      p.base[o + t] = wb;
      p.inter[o + t] = wi;
      p.uni[o + t] = wu;
    }
    last_c = bc, last_j = bjn;
  }
  if (lane == 0) p.n_nbr[row] = t;
}

}  // namespace anr
