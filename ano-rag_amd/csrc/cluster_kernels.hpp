// Device kernels of anr_index_dbscan (cluster.hip): DBSCAN over the stored rows of a flat index, as the closed form of
// sklearn's DBSCAN.fit_predict.  The eps-neighbourhood pairs are consumed where the MFMA tile walk of the
// self join (join_tile_mma, join_tile.hpp) produces them; nothing but O(N) arrays and the list of pairs the f16 image
// cannot decide is ever stored.
#pragma once
#include "common.hpp"
#include "join_tile.hpp"

namespace anr {

constexpr unsigned kNoRoot = 0xffffffffu;
enum { kDbDegree = 0, kDbUnion = 1, kDbBorder = 2 };
enum { kBlkCore = 1, kBlkNonCore = 2 };  // per 256-row block: holds a core row / a row that is not core

// counters of one run, device side
enum { kDbCand = 0, kDbResolvedIn = 1, kDbCore = 2, kDbClusters = 3, kDbNoise = 4, kDbChanged = 5, kDbCounters = 8 };

struct DbscanWalk {
  const uint4 *x16;
  const float *rowbias;   // L2: -0.5 ||x||^2 per row; nullptr on a cosine index
  int kb;
  int64_t n_rows, n_tiles;
  PatchGrid pg;
  int64_t n_slots;
  // w = x16_i . x16_j (+ rowbias_i + rowbias_j): -D^2 / 2 (L2) or 1 - D (cosine).  w > thr_hi: inside eps for certain;
  // w < thr_lo: outside for certain; between: the pair is re-scored from the float32 rows
  float thr_hi, thr_lo;
  unsigned *count;        // degree pass: eps-neighbours per row (the row itself not counted); later passes: 1 = core row
  const unsigned *blk;    // [blocks of 256 rows] kBlkCore | kBlkNonCore (union and border pass)
  unsigned *parent;       // union-find forest over the rows: parent[i] <= i, a root is its component's smallest row
  unsigned *border;       // smallest root among the core neighbours of a row that is not core (kNoRoot: none)
  uint2 *cand;            // degree pass: the undecided pairs (i < j)
  unsigned long long cap;
  unsigned long long *counters;
};

__device__ __forceinline__ unsigned uf_load(const unsigned *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned uf_find(const unsigned *parent, unsigned x) {
  for (unsigned p; (p = uf_load(parent + x)) != x;) x = p;  // parent[x] <= x: the walk ends
  return x;
}
// Lock-free union: the larger root is hooked under the smaller with atomicMin.  If `a` stopped being a root in the
// meantime the minimum may replace its parent `old` by `b`; uniting `old` with `b` next restores what that link said, and
// the values only fall, so the loop ends.  Whatever the order of the atomics, a component's root ends as its smallest row.
__device__ __noinline__ void uf_unite(unsigned *parent, unsigned a, unsigned b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const unsigned t = a;
      a = b;
      b = t;
    }
    const unsigned old = atomicMin(parent + a, b);
    if (old == a) return;
    a = old;
  }
}

// One walk of the upper triangle of 256 x 256 block pairs.  PASS kDbDegree counts the certain neighbours of both rows of
// every pair (reduced per row inside the tile: one global atomic per row and tile) and lists the undecided pairs;
// kDbUnion unites the two core rows of every certain pair; kDbBorder gives a row that is not core the smallest root among
// its core neighbours.  The diagonal block computes both orders of its pairs and keeps i < j, like the rest.
template <int PASS>
__global__ __launch_bounds__(512) void k_dbscan_walk(DbscanWalk p) {
  constexpr int TM = 8, TN = 8;
  extern __shared__ uint4 lds[];  // join_tile_mma's 128 KiB
  __shared__ float s_bj[256];     // rowbias of the j rows
  __shared__ unsigned s_a[512];   // per row of the tile pair, i rows then j rows: counts / roots
  __shared__ unsigned s_b[512];   // border pass: smallest core neighbour root found in this tile
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n_rows = (int)p.n_rows;
  for (int64_t slot = blockIdx.x; slot < p.n_slots; slot += gridDim.x) {
    int bi, bj;
    if (!patch_tile(p.pg, slot, bi, bj) || bi > bj) continue;
    if (PASS == kDbUnion && !((p.blk[bi] & kBlkCore) && (p.blk[bj] & kBlkCore))) continue;
    if (PASS == kDbBorder && !(((p.blk[bi] & kBlkNonCore) && (p.blk[bj] & kBlkCore)) ||
                               ((p.blk[bi] & kBlkCore) && (p.blk[bj] & kBlkNonCore))))
      continue;
    const int64_t tb0 = (int64_t)bi * TM, nb0 = (int64_t)bj * TN;
    const int wm = wave >> 1, wn = wave & 1;
    {
      // per-row state of the 256 + 256 rows, one row per thread (visible after the barriers of the product below)
      const int t = threadIdx.x;
      const int row = t < 256 ? (int)tb0 * 32 + t : (int)nb0 * 32 + t - 256;
      const bool live = row < n_rows;
      if (t >= 256) s_bj[t - 256] = (p.rowbias && live) ? p.rowbias[row] : 0.f;
      if (PASS == kDbDegree) s_a[t] = 0u;
      if (PASS == kDbUnion) {
        unsigned r = kNoRoot;
        if (live && p.count[row]) {
          r = uf_find(p.parent, (unsigned)row);
          if (r < uf_load(p.parent + row)) atomicMin(p.parent + row, r);  // keep the trees flat
        }
        s_a[t] = r;
      }
      if (PASS == kDbBorder) {
        s_a[t] = (live && p.count[row]) ? p.parent[row] : kNoRoot;  // roots are final here
        s_b[t] = kNoRoot;
      }
    }
    floatx16 acc[2][4];
    join_tile_mma(p.x16, p.kb, p.n_tiles, tb0, nb0, lds, lane, wave, acc);

    // masks over r of the pairs (i < j < n) that are certain neighbours / undecided
    unsigned in[2][4], un[2][4];
    float rbi[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int gi = (int)(tb0 + 2 * wm + m) * 32 + (lane & 31);
      rbi[m] = (p.rowbias && gi < n_rows) ? p.rowbias[gi] : 0.f;
    }
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int lj0 = (4 * wn + n) * 32 + 4 * (lane >> 5);
      float bjv[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 v = *reinterpret_cast<const float4 *>(&s_bj[lj0 + 8 * q]);
        bjv[4 * q] = v.x; bjv[4 * q + 1] = v.y; bjv[4 * q + 2] = v.z; bjv[4 * q + 3] = v.w;
      }
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const int gi = (int)(tb0 + 2 * wm + m) * 32 + (lane & 31);
        const int gj0 = (int)nb0 * 32 + lj0;
        unsigned valid = 0, hi = 0, lo = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int gj = gj0 + (r & 3) + 8 * (r >> 2);
          const float w = (acc[m][n][r] + rbi[m]) + bjv[r];
          valid |= (gi < gj && gj < n_rows) ? (1u << r) : 0u;
          hi |= (w > p.thr_hi) ? (1u << r) : 0u;
          lo |= (w >= p.thr_lo) ? (1u << r) : 0u;
        }
        in[m][n] = hi & valid;
        un[m][n] = lo & ~hi & valid;
      }
    }

    if (PASS == kDbDegree) {
      // rows i: a lane owns one row per m; the two waves of a row band meet in LDS
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        unsigned c = 0;
#pragma unroll
        for (int n = 0; n < 4; ++n) c += (unsigned)__popc(in[m][n]);
        if (c) atomicAdd(&s_a[(2 * wm + m) * 32 + (lane & 31)], c);
      }
      // rows j: bit r of the 32 lanes of a half wave is one column; ballots count it
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        if (__ballot((in[0][n] | in[1][n]) != 0u) == 0ull) continue;
        unsigned mine = 0;
#pragma unroll 1
        for (int r = 0; r < 16; ++r) {  // kept rolled: unrolled, the 128 ballots of a wave spill its scalar registers
          const unsigned long long b0 = __ballot((in[0][n] >> r) & 1u), b1 = __ballot((in[1][n] >> r) & 1u);
          const unsigned c_lo = (unsigned)(__popc((unsigned)b0) + __popc((unsigned)b1));
          const unsigned c_hi = (unsigned)(__popc((unsigned)(b0 >> 32)) + __popc((unsigned)(b1 >> 32)));
          const int col = (r & 3) + 8 * (r >> 2);
          if (lane == col) mine = c_lo;
          if (lane == col + 4) mine = c_hi;
        }
        if (lane < 32 && mine) atomicAdd(&s_a[256 + (4 * wn + n) * 32 + lane], mine);
      }
      // undecided pairs: one reservation per wave
      unsigned nun = 0;
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) nun += (unsigned)__popc(un[m][n]);
      if (__ballot(nun != 0u) != 0ull) {
        unsigned incl = nun;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const unsigned v = __shfl_up(incl, off);
          if (lane >= off) incl += v;
        }
        unsigned long long base = 0;
        if (lane == 63) base = atomicAdd(p.counters + kDbCand, (unsigned long long)incl);
        unsigned long long k = __shfl(base, 63) + (incl - nun);
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int n = 0; n < 4; ++n) {
            const unsigned gi = (unsigned)((tb0 + 2 * wm + m) * 32 + (lane & 31));
            const unsigned gj0 = (unsigned)((nb0 + 4 * wn + n) * 32 + 4 * (lane >> 5));
            unsigned h = un[m][n];
            while (h) {
              const int r = __ffs(h) - 1;
              h &= h - 1;
              if (k < p.cap) p.cand[k] = make_uint2(gi, gj0 + (r & 3) + 8 * (r >> 2));
              ++k;
            }
          }
      }
      __syncthreads();
      {
        const int t = threadIdx.x;
        const int row = t < 256 ? (int)tb0 * 32 + t : (int)nb0 * 32 + t - 256;
        if (s_a[t]) atomicAdd(p.count + row, s_a[t]);  // a counted row is < n
      }
    }

    if (PASS == kDbUnion) {
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        unsigned ri = s_a[(2 * wm + m) * 32 + (lane & 31)];
        if (ri == kNoRoot) continue;
        unsigned last = ri;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          unsigned h = in[m][n];
          while (h) {
            const int r = __ffs(h) - 1;
            h &= h - 1;
            const unsigned rj = s_a[256 + (4 * wn + n) * 32 + 4 * (lane >> 5) + (r & 3) + 8 * (r >> 2)];
            if (rj == kNoRoot || rj == ri || rj == last) continue;
            uf_unite(p.parent, ri, rj);
            last = rj;
            if (rj < ri) {  // the same component now: go on with its smaller row
              last = ri;
              ri = rj;
            }
          }
        }
      }
    }

    if (PASS == kDbBorder) {
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const int li = (2 * wm + m) * 32 + (lane & 31);
        const unsigned ri = s_a[li];
        unsigned best = kNoRoot;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          unsigned h = in[m][n];
          while (h) {
            const int r = __ffs(h) - 1;
            h &= h - 1;
            const int lj = 256 + (4 * wn + n) * 32 + 4 * (lane >> 5) + (r & 3) + 8 * (r >> 2);
            const unsigned rj = s_a[lj];
            if (ri == kNoRoot && rj != kNoRoot) best = rj < best ? rj : best;
            if (ri != kNoRoot && rj == kNoRoot) atomicMin(&s_b[lj], ri);
          }
        }
        if (best != kNoRoot) atomicMin(&s_b[li], best);
      }
      __syncthreads();
      {
        const int t = threadIdx.x;
        const int row = t < 256 ? (int)tb0 * 32 + t : (int)nb0 * 32 + t - 256;
        if (s_b[t] != kNoRoot) atomicMin(p.border + row, s_b[t]);
      }
    }
    __syncthreads();  // the per-row state is rewritten by the next tile pair
  }
}

// the float64 decision D <= eps of one listed pair, from the float32 rows: a wave takes 64 pairs at a time
struct DbscanResolve {
  const float *x32;
  int dim, l2;
  const uint2 *cand;
  unsigned long long n_cand;
  double eps;
  unsigned *count;
  uint2 *in_pairs;  // the pairs that are neighbours, compacted
  unsigned long long *counters;
};

__global__ __launch_bounds__(256) void k_dbscan_resolve(DbscanResolve p) {
  const int lane = threadIdx.x & 63;
  const unsigned long long w0 = (unsigned long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const unsigned long long wt = (unsigned long long)gridDim.x * 4;
  for (unsigned long long c0 = w0 * 64; c0 < p.n_cand; c0 += wt * 64) {
    const int nb = p.n_cand - c0 < 64 ? (int)(p.n_cand - c0) : 64;
    const uint2 my = lane < nb ? p.cand[c0 + lane] : make_uint2(0u, 0u);
    double mine = 0.0;
    for (int c = 0; c < nb; ++c) {
      const unsigned ri = __shfl(my.x, c), rj = __shfl(my.y, c);
      const float *a = p.x32 + (int64_t)ri * p.dim, *b = p.x32 + (int64_t)rj * p.dim;
      double acc = 0.0;
      if (p.l2) {
        for (int k = lane; k < p.dim; k += 64) {
          const double d = (double)a[k] - (double)b[k];
          acc += d * d;
        }
      } else {
        for (int k = lane; k < p.dim; k += 64) acc += (double)a[k] * (double)b[k];
      }
      for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
      if (lane == c) mine = p.l2 ? sqrt(acc) : 1.0 - acc;
    }
    const bool keep = lane < nb && mine <= p.eps;
    const unsigned long long mask = __ballot(keep);
    if (mask) {
      unsigned long long base = 0;
      if (lane == 0) base = atomicAdd(p.counters + kDbResolvedIn, (unsigned long long)__popcll(mask));
      base = __shfl(base, 0);
      if (keep) {
        p.in_pairs[base + __popcll(mask & ((1ull << lane) - 1ull))] = my;  // as long as the candidate list: it fits
        atomicAdd(p.count + my.x, 1u);
        atomicAdd(p.count + my.y, 1u);
      }
    }
  }
}

struct DbscanRows {
  int64_t n;
  int min_samples;
  unsigned *count, *blk, *parent, *border, *rank;
  int *labels;
  const uint2 *in_pairs;
  unsigned long long n_pairs;
  unsigned long long *counters;
};

// counts -> core flags (the row itself is in its neighbourhood), singleton forest, block summaries
__global__ __launch_bounds__(256) void k_dbscan_core(DbscanRows p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // a block is one 256-row block of the tile walk
  bool core = false;
  if (i < p.n) {
    core = (long long)p.count[i] + 1 >= (long long)p.min_samples;
    p.count[i] = core ? 1u : 0u;
    p.parent[i] = (unsigned)i;
    p.border[i] = kNoRoot;
  }
  const int ncore = __syncthreads_count(core), nnot = __syncthreads_count(i < p.n && !core);
  if (threadIdx.x == 0) {
    p.blk[blockIdx.x] = (ncore ? kBlkCore : 0u) | (nnot ? kBlkNonCore : 0u);
    if (ncore) atomicAdd(p.counters + kDbCore, (unsigned long long)ncore);
  }
}

__global__ __launch_bounds__(256) void k_dbscan_list_union(DbscanRows p) {
  for (unsigned long long k = (unsigned long long)blockIdx.x * 256 + threadIdx.x; k < p.n_pairs;
       k += (unsigned long long)gridDim.x * 256) {
    const uint2 e = p.in_pairs[k];
    if (p.count[e.x] && p.count[e.y]) uf_unite(p.parent, e.x, e.y);
  }
}

// one round of pointer jumping; counters[kDbChanged] is raised while some row is not yet attached to its root
__global__ __launch_bounds__(256) void k_dbscan_jump(DbscanRows p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.n) return;
  const unsigned q = uf_load(p.parent + i);
  const unsigned g = uf_load(p.parent + q);
  if (g != q) {
    atomicMin(p.parent + i, g);
    p.counters[kDbChanged] = 1ull;
  }
}

__global__ __launch_bounds__(256) void k_dbscan_list_border(DbscanRows p) {
  for (unsigned long long k = (unsigned long long)blockIdx.x * 256 + threadIdx.x; k < p.n_pairs;
       k += (unsigned long long)gridDim.x * 256) {
    const uint2 e = p.in_pairs[k];
    const bool ci = p.count[e.x] != 0u, cj = p.count[e.y] != 0u;
    if (ci && !cj) atomicMin(p.border + e.y, p.parent[e.x]);
    if (cj && !ci) atomicMin(p.border + e.x, p.parent[e.y]);
  }
}

// rank of every root among the roots, in row order (one workgroup: an exclusive scan in chunks of 1024 rows)
__global__ __launch_bounds__(1024) void k_dbscan_rank(DbscanRows p) {
  __shared__ unsigned s_w[16];
  __shared__ unsigned s_carry;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) s_carry = 0u;
  __syncthreads();
  for (int64_t i0 = 0; i0 < p.n; i0 += 1024) {
    const int64_t i = i0 + threadIdx.x;
    const unsigned f = (i < p.n && p.count[i] && p.parent[i] == (unsigned)i) ? 1u : 0u;
    const unsigned long long b = __ballot(f);
    if (lane == 0) s_w[wave] = (unsigned)__popcll(b);
    __syncthreads();
    unsigned before = s_carry;
    for (int w = 0; w < wave; ++w) before += s_w[w];
    if (i < p.n) p.rank[i] = before + (unsigned)__popcll(b & ((1ull << lane) - 1ull));
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned tot = 0;
      for (int w = 0; w < 16; ++w) tot += s_w[w];
      s_carry += tot;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) p.counters[kDbClusters] = s_carry;
}

__global__ __launch_bounds__(256) void k_dbscan_labels(DbscanRows p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int lab = -1;
  if (i < p.n) {
    const unsigned root = p.count[i] ? p.parent[i] : p.border[i];
    if (root != kNoRoot) lab = (int)p.rank[root];
    p.labels[i] = lab;
  }
  const int noise = __syncthreads_count(i < p.n && lab < 0);
  if (threadIdx.x == 0 && noise) atomicAdd(p.counters + kDbNoise, (unsigned long long)noise);
}

}  // namespace anr
