// anr_index_kmeans (include/anorag.h): sklearn's KMeans(n_clusters, n_init, random_state).fit on the stored float32 rows
// of an L2 index that does not normalise — the `kmeans` branch of the reference's TopicClustering._cpu_clustering, its
// _find_optimal_k and its _fallback_clustering (doc/clustering.py:80-87, 101-108, 110-134).  k-means++ seeding with the
// host's random draws, Lloyd iterations with sklearn's two stopping rules, best of n_init.  Everything that decides
// anything is float64 in one fixed order: distances |x|^2 + |c|^2 - 2 x.c with x.c (and both norms) from
// v_mfma_f64_16x16x4_f64 in ascending k; sums over rows in fixed blocks (a 256-leaf tree per block, blocks in ascending
// order); no floating-point atomics.  gram_f64.hpp has the MFMA lane map, DESIGN.md §5j the kernels, the orders and the
// byte counts;
// tests/kmeans_ref.py restates the orders in numpy.  Compiled without multiply-add contraction (Makefile, EXACT).
#include <algorithm>
#include <climits>
#include <cmath>
#include <mutex>
#include <vector>

#include "common.hpp"
#include "gram_f64.hpp"
#include "graph.hpp"

using namespace anr;

namespace {

constexpr int kKmMaxK = 64;      // centres of one call: four 16-column MFMA blocks
constexpr int kKmMaxTrials = 8;  // candidates of a seeding step: 2 + int(ln 64) = 6
constexpr int kKmTile = 64;      // rows of a distance workgroup: 4 waves of 16 rows
constexpr int kKmKC = 64;        // k-chunk staged through LDS
constexpr int kKmLdA = 68;       // floats per LDS row: (lane & 15) * 68 + (lane >> 4) hits 64 banks
constexpr int kKmLdC = 68;       // doubles per LDS centre row: 4 (lane & 15) + (lane >> 4) mod 32, the two-pass minimum of a 64-bit read
constexpr int kKmNT = 256;
constexpr int kKmBlock = 256;    // leaves of a sum tree / elements of a scan block
constexpr int kKmChunk = 512;    // rows of one update partial
constexpr int kKmSlab = 128;     // dimensions of one update workgroup

// state the host reads once per Lloyd iteration
struct KmCtrl {
  double pot;      // seeding: the current potential
  double shift;    // sum over centres of |c_new - c_old|^2
  double tol;      // tol_scale * mean per-dimension variance
  double inertia;  // sum over rows of |x - c_label|^2
  int best;        // seeding: the winning candidate of the step
  int empty;       // a centre without rows was met
  unsigned nchanged;
  int pad;
};

// |m_i|^2 of the rows of M, each as the diagonal of an MFMA product of 16 rows with themselves: the very sequence of
// operations that gives x.c in k_km_dist when c holds the same numbers, so a row and a centre taken from it are at
// distance exactly 0.  k in ascending steps of 4, zeros beyond dim.
template <typename T>
__global__ __launch_bounds__(kKmNT) void k_km_selfnorm(const T *__restrict__ M, int m, int dim, double *__restrict__ out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int row = blockIdx.x * kKmTile + w * 16 + (lane & 15);
  double4_t acc{0.0, 0.0, 0.0, 0.0};
  for (int ks = 0; ks < dim; ks += 4) {
    const int kk = ks + (lane >> 4);
    const double a = (row < m && kk < dim) ? (double)M[(int64_t)row * dim + kk] : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, a, acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if ((lane & 15) == (lane >> 4) + 4 * r && row < m) out[row] = acc[r];
}

struct KmDist {
  const float *x32;
  int dim, n;
  const double *cen;  // [kc][dim] centres or candidate rows
  const double *cn;   // [kc] their squared norms (k_km_selfnorm)
  int kc;
  const double *nx;   // [n] squared norms of the rows
  // assignment
  const int *old_labels;
  int *labels;
  KmCtrl *ctrl;
  // seeding
  const double *closest;  // [n]
  double *candd;          // [kc][n] min(closest, distance to candidate)
  int first;              // 1: there is no closest distance yet
};

// Distances of 64 rows to all centres.  Wave w owns rows 16 w .. 16 w + 15 and every 16-centre block (the lane map of
// gram_f64.hpp): result register r of block b is row 16 w + (lane >> 4) + 4 r, centre 16 b + (lane & 15).  SEED = false:
// the nearest centre of every row, ties to the lower index (per lane over its blocks in ascending order with <, then a
// xor butterfly over the 16 lanes of a row comparing (distance, index)), and the number of rows whose label changed (an
// integer atomic).  SEED = true: min(closest, max(distance, 0)) per candidate.
template <bool SEED>
__global__ __launch_bounds__(kKmNT) void k_km_dist(KmDist p) {
  __shared__ float As[kKmTile][kKmLdA];
  __shared__ double Cs[kKmMaxK][kKmLdC];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int i0 = blockIdx.x * kKmTile, nblk = (p.kc + 15) >> 4;
  double4_t acc[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) acc[b] = double4_t{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < p.dim; k0 += kKmKC) {
    for (int e = tid; e < kKmTile * kKmKC; e += kKmNT) {
      const int r = e / kKmKC, k = e % kKmKC, kk = k0 + k, row = i0 + r;
      As[r][k] = (row < p.n && kk < p.dim) ? p.x32[(int64_t)row * p.dim + kk] : 0.f;
    }
    for (int e = tid; e < nblk * 16 * kKmKC; e += kKmNT) {
      const int c = e / kKmKC, k = e % kKmKC, kk = k0 + k;
      Cs[c][k] = (c < p.kc && kk < p.dim) ? p.cen[(int64_t)c * p.dim + kk] : 0.0;
    }
    __syncthreads();
#pragma unroll 4
    for (int ks = 0; ks < kKmKC; ks += 4) {
      const double a = (double)As[w * 16 + (lane & 15)][ks + (lane >> 4)];
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (b < nblk) {
          const double bv = Cs[b * 16 + (lane & 15)][ks + (lane >> 4)];
          acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, acc[b], 0, 0, 0);
        }
    }
    __syncthreads();
  }
  unsigned changed = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = i0 + w * 16 + (lane >> 4) + 4 * r;
    const double nxr = row < p.n ? p.nx[row] : 0.0;
    if (SEED) {
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int col = b * 16 + (lane & 15);
        if (b < nblk && col < p.kc && row < p.n) {
          double d2 = (nxr + p.cn[col]) - 2.0 * acc[b][r];
          d2 = d2 > 0.0 ? d2 : 0.0;
          if (!p.first) {
            const double cl = p.closest[row];
            d2 = cl < d2 ? cl : d2;
          }
          p.candd[(int64_t)col * p.n + row] = d2;
        }
      }
    } else {
      double best = INFINITY;
      int bi = kKmMaxK;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int col = b * 16 + (lane & 15);
        if (b < nblk && col < p.kc) {
          const double d2 = (nxr + p.cn[col]) - 2.0 * acc[b][r];
          if (d2 < best) {
            best = d2;
            bi = col;
          }
        }
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        const double ob = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        if (ob < best || (ob == best && oi < bi)) {
          best = ob;
          bi = oi;
        }
      }
      if (bi >= p.kc) bi = 0;  // no finite distance (a NaN row): any label, but a valid one
      if ((lane & 15) == 0 && row < p.n) {
        if (p.old_labels[row] != bi) ++changed;
        p.labels[row] = bi;
      }
    }
  }
  if (!SEED && changed) atomicAdd(&p.ctrl->nchanged, changed);
}

// inclusive scan of one block of 256 values: eight Hillis-Steele steps (offsets 1, 2, .. 128), zeros beyond n
__global__ __launch_bounds__(kKmBlock) void k_km_scan(const double *__restrict__ v, int n, double *__restrict__ local,
                                                      double *__restrict__ blocktot) {
  __shared__ double sh[kKmBlock];
  const int tid = threadIdx.x, i = blockIdx.x * kKmBlock + tid;
  sh[tid] = i < n ? v[i] : 0.0;
  __syncthreads();
  for (int o = 1; o < kKmBlock; o <<= 1) {
    const double t = tid >= o ? sh[tid - o] : 0.0;
    __syncthreads();
    if (tid >= o) sh[tid] = sh[tid] + t;
    __syncthreads();
  }
  if (i < n) local[i] = sh[tid];
  if (tid == kKmBlock - 1) blocktot[blockIdx.x] = sh[tid];
}

// the blocks' offsets, one after the other; the step's candidates start at the clip value n - 1
__global__ void k_km_offsets(const double *blocktot, int nb, double *blockoff, int *cand, int trials, int n) {
  if (blockIdx.x || threadIdx.x) return;
  double s = 0.0;
  for (int b = 0; b < nb; ++b) {
    blockoff[b] = s;
    s = s + blocktot[b];
  }
  for (int t = 0; t < trials; ++t) cand[t] = n - 1;
}

// searchsorted(cumsum, u * pot, side='left') clipped to n - 1: the first row whose cumulative sum reaches the value.  A row
// reports itself when it reaches the value and its predecessor does not; the smallest such row is the answer whether or
// not rounding left the sums monotone (integer atomicMin).
__global__ void k_km_search(const double *__restrict__ local, const double *__restrict__ blockoff, int n,
                            const double *__restrict__ u, int trials, const KmCtrl *ctrl, int *cand) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double cs = blockoff[i / kKmBlock] + local[i];
  const double prev = i > 0 ? blockoff[(i - 1) / kKmBlock] + local[i - 1] : 0.0;
  const double pot = ctrl->pot;
  for (int t = 0; t < trials; ++t) {
    const double rv = u[t] * pot;
    if (cs >= rv && (i == 0 || !(prev >= rv))) atomicMin(&cand[t], i);
  }
}

// out[t][:] = the stored row ids[t], widened
__global__ void k_km_gather(const float *__restrict__ x32, int dim, const int *__restrict__ ids, double *__restrict__ out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
  if (j < dim) out[(int64_t)t * dim + j] = (double)x32[(int64_t)ids[t] * dim + j];
}

// part[t][block] = the sum of 256 consecutive values of v[t][:] by a halving tree (leaf i + leaf i + o for o = 128, 64, .. 1)
__global__ __launch_bounds__(kKmBlock) void k_km_blocksum(const double *__restrict__ v, int n, double *__restrict__ part) {
  __shared__ double sh[kKmBlock];
  const int tid = threadIdx.x, i = blockIdx.x * kKmBlock + tid, t = blockIdx.y;
  sh[tid] = i < n ? v[(int64_t)t * n + i] : 0.0;
  __syncthreads();
  for (int o = kKmBlock / 2; o >= 1; o >>= 1) {
    if (tid < o) sh[tid] = sh[tid] + sh[tid + o];
    __syncthreads();
  }
  if (tid == 0) part[(int64_t)t * gridDim.x + blockIdx.x] = sh[0];
}

// the totals of `trials` rows of partials, each summed in ascending order; the first smallest total wins.  step >= 0: a
// seeding step (the winner's row becomes centre `step`, its total the potential); step < 0: one total, written to *out.
__global__ void k_km_pick(const double *part, int np, int trials, int step, const int *cand, int *centre_ids, KmCtrl *ctrl,
                          double *out) {
  if (blockIdx.x || threadIdx.x) return;
  double bestv = 0.0;
  int best = 0;
  for (int t = 0; t < trials; ++t) {
    double s = 0.0;
    for (int b = 0; b < np; ++b) s = s + part[(int64_t)t * np + b];
    if (t == 0 || s < bestv) {
      bestv = s;
      best = t;
    }
  }
  if (step >= 0) {
    ctrl->pot = bestv;
    ctrl->best = best;
    centre_ids[step] = cand[best];
  } else {
    *out = bestv;
  }
}

__global__ void k_km_take(const double *__restrict__ candd, int n, const KmCtrl *ctrl, double *__restrict__ closest) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) closest[i] = candd[(int64_t)ctrl->best * n + i];
}

__global__ void k_km_set_first(int *cand, const int *first_row) {
  if (blockIdx.x == 0 && threadIdx.x == 0) cand[0] = *first_row;
}

// Per chunk of 512 rows and per centre: the sum of the chunk's rows with that label, rows in ascending order, one thread per
// dimension with its k running sums in its own LDS column.  SQ = true: (x - mean)^2 in place of x (labels == nullptr: one
// centre, every row).  Workgroups of slab 0 also count the chunk's rows per centre.
template <bool SQ>
__global__ __launch_bounds__(kKmSlab) void k_km_colsum(const float *__restrict__ x32, int dim, int n, const int *__restrict__ labels,
                                                       int k, const double *__restrict__ mean, double *__restrict__ partial,
                                                       int *__restrict__ cntpart) {
  extern __shared__ double acc[];  // [k][kKmSlab]
  const int tid = threadIdx.x, j = blockIdx.y * kKmSlab + tid;
  const int r0 = blockIdx.x * kKmChunk, r1 = min(r0 + kKmChunk, n);
  for (int c = 0; c < k; ++c) acc[c * kKmSlab + tid] = 0.0;
  if (j < dim) {
    const double mu = SQ ? mean[j] : 0.0;
    for (int r = r0; r < r1; ++r) {
      int lab = labels ? labels[r] : 0;
      if ((unsigned)lab >= (unsigned)k) lab = 0;
      const double xv = (double)x32[(int64_t)r * dim + j];
      const double val = SQ ? (xv - mu) * (xv - mu) : xv;
      acc[lab * kKmSlab + tid] = acc[lab * kKmSlab + tid] + val;
    }
    for (int c = 0; c < k; ++c) partial[((int64_t)blockIdx.x * k + c) * dim + j] = acc[c * kKmSlab + tid];
  }
  if (blockIdx.y == 0 && cntpart)
    for (int c = tid; c < k; c += kKmSlab) {
      int cnt = 0;
      for (int r = r0; r < r1; ++r) cnt += (labels ? labels[r] : 0) == c;
      cntpart[(int64_t)blockIdx.x * k + c] = cnt;
    }
}

// out[j] = (the chunks' partials of column j, added in ascending order) / n
__global__ void k_km_colreduce(const double *__restrict__ partial, int nchunks, int dim, int n, double *__restrict__ out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= dim) return;
  double s = 0.0;
  for (int ch = 0; ch < nchunks; ++ch) s = s + partial[(int64_t)ch * dim + j];
  out[j] = s / (double)n;
}

// new centre = (the chunks' partials, added in ascending order) / count; a centre without rows keeps its place and raises
// ctrl->empty
__global__ void k_km_centres(const double *__restrict__ partial, const int *__restrict__ cntpart, int nchunks, int k, int dim,
                             const double *__restrict__ cold, double *__restrict__ cnew, KmCtrl *ctrl) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= k * dim) return;
  const int c = e / dim, j = e % dim;
  double s = 0.0;
  int64_t cnt = 0;
  for (int ch = 0; ch < nchunks; ++ch) {
    s = s + partial[((int64_t)ch * k + c) * dim + j];
    cnt += cntpart[(int64_t)ch * k + c];
  }
  if (cnt == 0) {
    ctrl->empty = 1;
    cnew[e] = cold[e];
  } else {
    cnew[e] = s / (double)cnt;
  }
}

// shift = sum over centres (ascending) of the sum over dimensions (ascending) of (c_new - c_old)^2
__global__ __launch_bounds__(kKmMaxK) void k_km_shift(const double *__restrict__ cold, const double *__restrict__ cnew, int k,
                                                      int dim, KmCtrl *ctrl) {
  __shared__ double sh[kKmMaxK];
  const int c = threadIdx.x;
  double s = 0.0;
  if (c < k)
    for (int j = 0; j < dim; ++j) {
      const double df = cnew[(int64_t)c * dim + j] - cold[(int64_t)c * dim + j];
      s = s + df * df;
    }
  sh[c] = s;
  __syncthreads();
  if (c == 0) {
    double t = 0.0;
    for (int i = 0; i < k; ++i) t = t + sh[i];
    ctrl->shift = t;
  }
}

__global__ void k_km_tol(const double *var, int dim, double scale, KmCtrl *ctrl) {
  if (blockIdx.x || threadIdx.x) return;
  double s = 0.0;
  for (int j = 0; j < dim; ++j) s = s + var[j];
  ctrl->tol = scale * (s / (double)dim);
}

// v[i] = sum over dimensions (ascending) of (x_i - c_label(i))^2, a thread per row
__global__ void k_km_rowinertia(const float *__restrict__ x32, int dim, int n, const double *__restrict__ cen,
                                const int *__restrict__ labels, double *__restrict__ v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float *x = x32 + (int64_t)i * dim;
  const double *c = cen + (int64_t)labels[i] * dim;
  double s = 0.0;
  int j = 0;
  if ((dim & 3) == 0) {
    for (; j < dim; j += 4) {
      const float4 q = *reinterpret_cast<const float4 *>(x + j);
      const double d0 = (double)q.x - c[j], d1 = (double)q.y - c[j + 1], d2 = (double)q.z - c[j + 2], d3 = (double)q.w - c[j + 3];
      s = s + d0 * d0;
      s = s + d1 * d1;
      s = s + d2 * d2;
      s = s + d3 * d3;
    }
  } else {
    for (; j < dim; ++j) {
      const double df = (double)x[j] - c[j];
      s = s + df * df;
    }
  }
  v[i] = s;
}

// everything one call needs, carved from the handle's arena
struct Plan {
  const float *x32;
  int n, dim, k, trials, nb, nsb, nchunks;
  hipStream_t st;
  double *nx, *closest, *local, *candd, *v, *blocktot, *blockoff, *part, *part2, *partial, *cen[2], *ccand, *cn, *mean, *var, *u;
  int *labels[2], *cntpart, *cand, *centre_ids, *first_rows;
  KmCtrl *ctrl;
};

#define KM_LAUNCH(kernel, grid, block, lds, ...)                        \
  do {                                                                  \
    hipLaunchKernelGGL(kernel, grid, block, lds, P.st, __VA_ARGS__);    \
    ANR_HIP(hipGetLastError());                                         \
  } while (0)

// sum of v[t][0 .. n) for t < trials in the fixed order: 256-leaf trees, 256-leaf trees of those, the rest one after the other
int ordered_sums(const Plan &P, const double *v, int trials, int step, double *out) {
  KM_LAUNCH(k_km_blocksum, dim3((unsigned)P.nb, (unsigned)trials), dim3(kKmBlock), 0, v, P.n, P.part);
  KM_LAUNCH(k_km_blocksum, dim3((unsigned)P.nsb, (unsigned)trials), dim3(kKmBlock), 0, P.part, P.nb, P.part2);
  KM_LAUNCH(k_km_pick, dim3(1), dim3(1), 0, P.part2, P.nsb, trials, step, P.cand, P.centre_ids, P.ctrl, out);
  return ANR_OK;
}

// distances of every row to the `kc` rows of `cen`
template <bool SEED>
int distances(const Plan &P, const double *cen, int kc, const int *old_labels, int *labels, int first) {
  KM_LAUNCH(k_km_selfnorm<double>, dim3((unsigned)ceil_div(kc, kKmTile)), dim3(kKmNT), 0, cen, kc, P.dim, P.cn);
  const KmDist d{P.x32, P.dim, P.n, cen, P.cn, kc, P.nx, old_labels, labels, P.ctrl, P.closest, P.candd, first};
  KM_LAUNCH(k_km_dist<SEED>, dim3((unsigned)ceil_div(P.n, kKmTile)), dim3(kKmNT), 0, d);
  return ANR_OK;
}

// sklearn's _kmeans_plusplus with the host's draws: centre 0 is the given row; every further centre is the best of
// `trials` rows drawn in proportion to the closest squared distance
int seed(const Plan &P, int init) {
  const unsigned g256 = (unsigned)ceil_div(P.n, 256);
  for (int c = 0; c < P.k; ++c) {
    int trials = 1;
    if (c == 0) {
      KM_LAUNCH(k_km_set_first, dim3(1), dim3(1), 0, P.cand, (const int *)P.first_rows + init);
    } else {
      trials = P.trials;
      KM_LAUNCH(k_km_scan, dim3((unsigned)P.nb), dim3(kKmBlock), 0, P.closest, P.n, P.local, P.blocktot);
      KM_LAUNCH(k_km_offsets, dim3(1), dim3(1), 0, P.blocktot, P.nb, P.blockoff, P.cand, trials, P.n);
      const double *u = P.u + ((int64_t)init * (P.k - 1) + (c - 1)) * P.trials;
      KM_LAUNCH(k_km_search, dim3(g256), dim3(256), 0, P.local, P.blockoff, P.n, u, trials, P.ctrl, P.cand);
    }
    KM_LAUNCH(k_km_gather, dim3((unsigned)ceil_div(P.dim, 256), (unsigned)trials), dim3(256), 0, P.x32, P.dim, (const int *)P.cand,
              P.ccand);
    ANR_TRY(distances<true>(P, P.ccand, trials, nullptr, nullptr, c == 0));
    ANR_TRY(ordered_sums(P, P.candd, trials, c, nullptr));
    KM_LAUNCH(k_km_take, dim3(g256), dim3(256), 0, P.candd, P.n, P.ctrl, P.closest);
  }
  return ANR_OK;
}

}  // namespace

extern "C" int anr_index_kmeans(anr_index *h, int32_t k, int32_t n_init, int32_t n_local_trials, const int64_t *first_rows,
                                const double *uniforms, int32_t max_iter, double tol_scale, int32_t *labels, double *centres,
                                double *inertia, int32_t *n_iter, int32_t *best_init, int64_t *stats) {
  if (!h) return fail(ANR_EINVAL, "null handle");
  const IndexCore c0 = index_core(h);
  if (c0.metric != ANR_METRIC_L2 || c0.normalize)
    return fail(ANR_EINVAL, "k-means needs an L2 index that stores its rows as given (no normalisation)");
  DeviceGuard g(c0.device);
  if (!g.ok) return fail(ANR_EHIP, "hipSetDevice(%d) failed", c0.device);
  std::lock_guard<std::mutex> lk(*c0.mu);
  const IndexCore cur = index_core(h);  // under the lock: an add may have moved the rows
  if (k < 2) return fail(ANR_EINVAL, "k-means: n_clusters = %d, at least 2 are needed", k);
  if (k > kKmMaxK) return fail(ANR_EINVAL, "k-means: n_clusters = %d is above the %d this kernel holds", k, kKmMaxK);
  if (cur.ntotal < k) return fail(ANR_EINVAL, "k-means: n_samples = %lld should be >= n_clusters = %d", (long long)cur.ntotal, k);
  if (cur.ntotal > (int64_t)INT_MAX - kKmChunk) return fail(ANR_EINVAL, "k-means: too many rows for one call");
  if (n_init < 1 || max_iter < 1) return fail(ANR_EINVAL, "k-means: n_init and max_iter must be at least 1");
  if (n_local_trials < 1 || n_local_trials > kKmMaxTrials)
    return fail(ANR_EINVAL, "k-means: %d local trials, 1 to %d are held", n_local_trials, kKmMaxTrials);
  if (!first_rows || !uniforms || !labels) return fail(ANR_EINVAL, "k-means: null first_rows, uniforms or labels");
  if (!(tol_scale >= 0.0)) return fail(ANR_EINVAL, "k-means: tol_scale must not be negative");
  const int n = (int)cur.ntotal, dim = cur.dim;
  std::vector<int> first((size_t)n_init);
  for (int i = 0; i < n_init; ++i) {
    if (first_rows[i] < 0 || first_rows[i] >= n) return fail(ANR_EINVAL, "k-means: first row %lld of init %d is not a row", (long long)first_rows[i], i);
    first[i] = (int)first_rows[i];
  }
  const size_t n_u = (size_t)n_init * (k - 1) * n_local_trials;
  for (size_t i = 0; i < n_u; ++i)
    if (!(uniforms[i] >= 0.0 && uniforms[i] <= 1.0)) return fail(ANR_EINVAL, "k-means: uniform %zu is outside [0, 1]", i);

  Plan P{};
  P.x32 = cur.x32, P.n = n, P.dim = dim, P.k = k, P.trials = n_local_trials, P.st = cur.stream;
  P.nb = (int)ceil_div(n, kKmBlock), P.nsb = (int)ceil_div(P.nb, kKmBlock), P.nchunks = (int)ceil_div(n, kKmChunk);
  const int tmax = std::max(1, (int)n_local_trials);
  ArenaLayout<256> L;
  const size_t N = (size_t)n;
  const size_t o_first = L.take((size_t)n_init * 4), o_u = L.take(n_u * 8), in_end = L.at;
  const size_t o_ctrl = L.take(sizeof(KmCtrl)), o_nx = L.take(N * 8), o_closest = L.take(N * 8), o_local = L.take(N * 8);
  const size_t o_candd = L.take(N * 8 * tmax), o_v = L.take(N * 8), o_btot = L.take((size_t)P.nb * 8);
  const size_t o_boff = L.take((size_t)P.nb * 8);
  const size_t o_part = L.take((size_t)P.nb * 8 * tmax), o_part2 = L.take((size_t)P.nsb * 8 * tmax);
  const size_t o_partial = L.take((size_t)P.nchunks * k * dim * 8), o_cnt = L.take((size_t)P.nchunks * k * 4);
  const size_t o_c0 = L.take((size_t)k * dim * 8), o_c1 = L.take((size_t)k * dim * 8);
  const size_t o_cc = L.take((size_t)kKmMaxTrials * dim * 8);
  const size_t o_cn = L.take(kKmMaxK * 8), o_mean = L.take((size_t)dim * 8), o_var = L.take((size_t)dim * 8);
  const size_t o_l0 = L.take(N * 4), o_l1 = L.take(N * 4), o_cand = L.take(kKmMaxTrials * 4), o_ids = L.take(kKmMaxK * 4);
  const size_t total = L.at;

  DevBuf<unsigned char> &arena = index_scratch(h).km_arena;
  ANR_TRY(arena.alloc((int64_t)total, "k-means", (int64_t)(total + total / 4)));
  unsigned char *A = arena.p;
  auto D = [&](size_t o) { return reinterpret_cast<double *>(A + o); };
  auto I = [&](size_t o) { return reinterpret_cast<int *>(A + o); };
  P.first_rows = I(o_first), P.u = D(o_u), P.ctrl = reinterpret_cast<KmCtrl *>(A + o_ctrl), P.nx = D(o_nx);
  P.closest = D(o_closest), P.local = D(o_local), P.candd = D(o_candd), P.v = D(o_v), P.blocktot = D(o_btot);
  P.blockoff = D(o_boff), P.part = D(o_part), P.part2 = D(o_part2), P.partial = D(o_partial), P.cntpart = I(o_cnt);
  P.cen[0] = D(o_c0), P.cen[1] = D(o_c1), P.ccand = D(o_cc), P.cn = D(o_cn), P.mean = D(o_mean), P.var = D(o_var);
  P.labels[0] = I(o_l0), P.labels[1] = I(o_l1), P.cand = I(o_cand), P.centre_ids = I(o_ids);
  hipStream_t st = P.st;

  std::vector<unsigned char> in(in_end, 0);
  memcpy(&in[o_first], first.data(), (size_t)n_init * 4);
  if (n_u) memcpy(&in[o_u], uniforms, n_u * 8);
  ANR_HIP(hipMemcpyAsync(A, in.data(), in_end, hipMemcpyHostToDevice, st));
  ANR_HIP(hipMemsetAsync(A + o_ctrl, 0, sizeof(KmCtrl), st));

  // once per call: the rows' squared norms, and tol from the per-dimension variances (two passes: mean, then deviations)
  const unsigned g256 = (unsigned)ceil_div(n, 256), gdim = (unsigned)ceil_div(dim, 256);
  const dim3 gcol((unsigned)P.nchunks, (unsigned)ceil_div(dim, kKmSlab));
  KM_LAUNCH(k_km_selfnorm<float>, dim3((unsigned)ceil_div(n, kKmTile)), dim3(kKmNT), 0, P.x32, n, dim, P.nx);
  KM_LAUNCH(k_km_colsum<false>, gcol, dim3(kKmSlab), (size_t)kKmSlab * 8, P.x32, dim, n, (const int *)nullptr, 1,
            (const double *)nullptr, P.partial, (int *)nullptr);
  KM_LAUNCH(k_km_colreduce, dim3(gdim), dim3(256), 0, P.partial, P.nchunks, dim, n, P.mean);
  KM_LAUNCH(k_km_colsum<true>, gcol, dim3(kKmSlab), (size_t)kKmSlab * 8, P.x32, dim, n, (const int *)nullptr, 1,
            (const double *)P.mean, P.partial, (int *)nullptr);
  KM_LAUNCH(k_km_colreduce, dim3(gdim), dim3(256), 0, P.partial, P.nchunks, dim, n, P.var);
  KM_LAUNCH(k_km_tol, dim3(1), dim3(1), 0, P.var, dim, tol_scale, P.ctrl);

  std::vector<int32_t> lab_host(N), best_labels;
  std::vector<double> cen_host((size_t)k * dim), best_centres;
  double best_inertia = 0.0;
  int best_iter = 0, best_i = -1, n_strict = 0;
  int64_t total_iters = 0, assign_passes = 0;
  KmCtrl ctrl{};
  for (int init = 0; init < n_init; ++init) {
    ANR_TRY(seed(P, init));
    int cur_c = 0, cur_l = 0;  // cen[cur_c]: the centres in force; labels[cur_l]: the previous iteration's labels
    KM_LAUNCH(k_km_gather, dim3(gdim, (unsigned)k), dim3(256), 0, P.x32, dim, P.centre_ids, P.cen[cur_c]);
    ANR_HIP(hipMemsetAsync(P.labels[cur_l], 0xff, N * 4, st));  // -1: no row keeps its label in iteration 0
    bool strict = false;
    int iters = 0;
    for (int it = 0; it < max_iter; ++it) {
      ANR_HIP(hipMemsetAsync(&P.ctrl->nchanged, 0, sizeof(unsigned), st));
      ANR_TRY(distances<false>(P, P.cen[cur_c], k, P.labels[cur_l], P.labels[cur_l ^ 1], 0));
      KM_LAUNCH(k_km_colsum<false>, gcol, dim3(kKmSlab), (size_t)k * kKmSlab * 8, P.x32, dim, n, (const int *)P.labels[cur_l ^ 1], k,
                (const double *)nullptr, P.partial, P.cntpart);
      KM_LAUNCH(k_km_centres, dim3((unsigned)ceil_div((int64_t)k * dim, 256)), dim3(256), 0, P.partial, P.cntpart, P.nchunks, k,
                dim, P.cen[cur_c], P.cen[cur_c ^ 1], P.ctrl);
      KM_LAUNCH(k_km_shift, dim3(1), dim3(kKmMaxK), 0, P.cen[cur_c], P.cen[cur_c ^ 1], k, dim, P.ctrl);
      ANR_HIP(hipMemcpyAsync(&ctrl, P.ctrl, sizeof(KmCtrl), hipMemcpyDeviceToHost, st));
      ANR_HIP(hipStreamSynchronize(st));
      ++total_iters, ++assign_passes;
      iters = it + 1;
      if (ctrl.empty) {
        if (stats) {
          std::fill(stats, stats + 8, (int64_t)0);
          stats[0] = total_iters, stats[1] = assign_passes, stats[3] = arena.cap, stats[5] = init;
        }
        return fail(ANR_EEMPTY, "k-means: a cluster lost all its rows (init %d, iteration %d); sklearn relocates such a "
                                "centre in an order that is not defined, so this input stays on sklearn", init, it);
      }
      cur_c ^= 1;  // the new centres are in force
      cur_l ^= 1;  // and this iteration's labels are the ones to compare with
      if (ctrl.nchanged == 0) {
        strict = true;
        break;
      }
      if (ctrl.shift <= ctrl.tol) break;
    }
    if (!strict) {  // the labels belong to the centres before the last update: once more against the final ones
      ANR_TRY(distances<false>(P, P.cen[cur_c], k, P.labels[cur_l], P.labels[cur_l ^ 1], 0));
      cur_l ^= 1;
      ++assign_passes;
    } else {
      ++n_strict;
    }
    KM_LAUNCH(k_km_rowinertia, dim3(g256), dim3(256), 0, P.x32, dim, n, (const double *)P.cen[cur_c], (const int *)P.labels[cur_l], P.v);
    ANR_TRY(ordered_sums(P, P.v, 1, -1, &P.ctrl->inertia));
    ANR_HIP(hipMemcpyAsync(&ctrl, P.ctrl, sizeof(KmCtrl), hipMemcpyDeviceToHost, st));
    ANR_HIP(hipMemcpyAsync(lab_host.data(), P.labels[cur_l], N * 4, hipMemcpyDeviceToHost, st));
    ANR_HIP(hipMemcpyAsync(cen_host.data(), P.cen[cur_c], (size_t)k * dim * 8, hipMemcpyDeviceToHost, st));
    ANR_HIP(hipStreamSynchronize(st));
    bool better = best_i < 0;
    if (!better && ctrl.inertia < best_inertia) {
      // sklearn's _is_same_clustering: the same partition under a renaming of the labels does not replace the best
      std::vector<int> map((size_t)k, -1);
      bool same = true;
      for (size_t i = 0; i < N && same; ++i) {
        int &m = map[(size_t)lab_host[i]];
        if (m == -1) m = best_labels[i];
        else if (m != best_labels[i]) same = false;
      }
      better = !same;
    }
    if (better) {
      best_labels = lab_host, best_centres = cen_host;
      best_inertia = ctrl.inertia, best_iter = iters, best_i = init;
    }
  }
  memcpy(labels, best_labels.data(), N * 4);
  if (centres) memcpy(centres, best_centres.data(), (size_t)k * dim * 8);
  if (inertia) *inertia = best_inertia;
  if (n_iter) *n_iter = best_iter;
  if (best_init) *best_init = best_i;
  if (stats) {
    std::fill(stats, stats + 8, (int64_t)0);
    stats[0] = total_iters;
    stats[1] = assign_passes;
    stats[2] = (int64_t)n_init * k;
    stats[3] = arena.cap;
    stats[4] = ceil_div(dim, kKmKC) * (kKmKC / 4);
    stats[5] = -1;
    stats[6] = n_strict;
    memcpy(&stats[7], &ctrl.tol, 8);
  }
  return ANR_OK;
}
