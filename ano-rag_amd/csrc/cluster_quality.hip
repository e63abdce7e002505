// anr_index_cluster_quality (include/anorag.h): the two quality measures of the reference's
// TopicClustering._analyze_clusters (doc/clustering.py:171-215) on the stored rows of an L2 index — sklearn's Euclidean
// silhouette of every row (the noise label -1 counted as a cluster) and, per cluster, the mean and the population
// standard deviation of scipy's cosine distance over its pairs.  Everything comes from one float64 Gram G = X X^T formed
// with the tile diversity.hip uses (gram_f64.hpp: the lane map and the determinism rule); the rows are first sorted by
// label with the stable radix sort, so that a label is a run of consecutive positions.  DESIGN.md §5h has the tile walk,
// the lane-to-row reduction and the error bounds.  Compiled without multiply-add contraction (Makefile, EXACT).
#include <algorithm>
#include <climits>
#include <cmath>
#include <limits>
#include <mutex>
#include <vector>

#include "common.hpp"
#include "gram_f64.hpp"
#include "graph.hpp"

using namespace anr;

namespace {

constexpr int kCqTile = 64;  // a workgroup's tile: 4 waves of 16 rows x 64 columns (four 16 x 16 MFMA blocks each)
constexpr int kCqLd = 68;    // row length in LDS: the 64 lanes of an operand read, (lane & 15) * 68 + (lane >> 4), hit 64 banks
constexpr int kCqNT = 256;

// Raw products of one 64 x 64 tile of G = X X^T, the rows named by ra (tile rows) and rb (tile columns), -1 = padding: the
// shared tile with 4 x 1 waves of four 16 x 16 blocks each.  Result register r of block b of wave w is row
// 16 w + (lane >> 4) + 4 r, column 16 b + (lane & 15).  Ends with a barrier.
__device__ __forceinline__ void cq_tile_gram(const float *__restrict__ x32, int dim, const int64_t *ra, const int64_t *rb,
                                             float (*As)[kCqLd], float (*Bs)[kCqLd], double4_t acc[4]) {
  gram_f64_tile<4, 1, 4, kCqLd>(x32, dim, ra, rb, As, Bs, acc);
}

// positions are places in the label-sorted order; perm[position] is the stored row
struct CqView {
  const float *x32;
  int dim, n;
  const unsigned *perm;  // [n]
};

__global__ void k_cq_keys(const int *labels, int n, unsigned long long *keys, unsigned *iota) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  keys[i] = (unsigned long long)((unsigned)labels[i] ^ 0x80000000u);  // ascending as signed integers
  iota[i] = (unsigned)i;
}

// G_pp of every position: the diagonal of the diagonal tiles of the same product loop
__global__ __launch_bounds__(kCqNT) void k_cq_norms(CqView v, double *nrm2) {
  __shared__ float As[kCqTile][kCqLd], Bs[kCqTile][kCqLd];
  __shared__ int64_t ra[kCqTile];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int i0 = blockIdx.x * kCqTile;
  if (tid < kCqTile) ra[tid] = i0 + tid < v.n ? (int64_t)v.perm[i0 + tid] : -1;
  __syncthreads();
  double4_t acc[4];
  cq_tile_gram(v.x32, v.dim, ra, ra, As, Bs, acc);
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (b == w && (lane & 15) == (lane >> 4) + 4 * r) {
        const int pos = i0 + w * 16 + (lane & 15);
        if (pos < v.n) nrm2[pos] = acc[b][r];
      }
}

struct CqSil {
  CqView v;
  const int *segpos;     // [n] label run (segment) of a position
  const int *seg_start;  // [n_seg + 1]
  const double *nrm2;    // [n] by position
  double *sil;           // [n] by stored row
};

// One workgroup per strip of 64 positions, a wave per 16 of them; the wave keeps its rows for the whole walk over the
// column tiles in sorted order.  Per 16-column block a lane holds D of its column for four rows; the 16 lanes of a row sum
// theirs by a fixed xor butterfly, masked to the label run in hand (a block can hold several runs: one pass each), and every
// lane adds the block's sum to its own copy of the row's running sum (compensated).  When the run changes the sum is closed:
// divided by the run's size and taken as a_i or into min b_i.  Which run is open depends on the column alone, so the whole
// wave branches together.  No atomics: s_i is one fixed sequence of operations.
__global__ __launch_bounds__(kCqNT) void k_cq_silhouette(CqSil p) {
  __shared__ float As[kCqTile][kCqLd], Bs[kCqTile][kCqLd];
  __shared__ int64_t ra[kCqTile], rb[kCqTile];
  __shared__ int cs[kCqTile];
  __shared__ double cn[kCqTile];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = p.v.n;
  const int i0 = blockIdx.x * kCqTile;
  if (tid < kCqTile) ra[tid] = i0 + tid < n ? (int64_t)p.v.perm[i0 + tid] : -1;
  int myseg[4];
  double gii[4], cur[4], comp[4], a[4], minb[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int pos = i0 + w * 16 + (lane >> 4) + 4 * r;
    myseg[r] = pos < n ? p.segpos[pos] : -2;
    gii[r] = pos < n ? p.nrm2[pos] : 0.0;
    cur[r] = comp[r] = a[r] = 0.0;
    minb[r] = INFINITY;
  }
  int open = -1;
  auto close = [&](int s) {
    const int m = p.seg_start[s + 1] - p.seg_start[s];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (myseg[r] == s) {
        a[r] = m > 1 ? cur[r] / (double)(m - 1) : 0.0;
      } else {
        const double b = cur[r] / (double)m;
        if (b < minb[r]) minb[r] = b;
      }
    }
  };
  for (int j0 = 0; j0 < n; j0 += kCqTile) {
    __syncthreads();  // the previous tile's epilogue has read cs and cn
    if (tid < kCqTile) {
      const int pos = j0 + tid;
      rb[tid] = pos < n ? (int64_t)p.v.perm[pos] : -1;
      cs[tid] = pos < n ? p.segpos[pos] : -1;
      cn[tid] = pos < n ? p.nrm2[pos] : 0.0;
    }
    __syncthreads();
    double4_t acc[4];
    cq_tile_gram(p.v.x32, p.v.dim, ra, rb, As, Bs, acc);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int c0 = j0 + b * 16;
      if (c0 < n) {
        const int sj = cs[b * 16 + (lane & 15)];
        const double gjj = cn[b * 16 + (lane & 15)];
        double D[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double d2 = gii[r] + gjj - 2.0 * acc[b][r];
          D[r] = sqrt(d2 > 0.0 ? d2 : 0.0);
        }
        const int s_first = cs[b * 16], s_last = cs[min(c0 + 15, n - 1) - j0];
        for (int s = s_first; s <= s_last; ++s) {
          if (s != open) {
            if (open >= 0) close(open);
            open = s;
#pragma unroll
            for (int r = 0; r < 4; ++r) cur[r] = comp[r] = 0.0;
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            double t = sj == s ? D[r] : 0.0;
            t += __shfl_xor(t, 1);
            t += __shfl_xor(t, 2);
            t += __shfl_xor(t, 4);
            t += __shfl_xor(t, 8);
            const double y = t - comp[r], z = cur[r] + y;
            comp[r] = (z - cur[r]) - y;
            cur[r] = z;
          }
        }
      }
    }
  }
  if (open >= 0) close(open);
  if ((lane & 15) == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int pos = i0 + w * 16 + (lane >> 4) + 4 * r;
      if (pos >= n) continue;
      const int m = p.seg_start[myseg[r] + 1] - p.seg_start[myseg[r]];
      double s = 0.0;  // a label of one row, no other label, or 0 / 0
      if (m > 1 && minb[r] != INFINITY) {
        const double den = a[r] > minb[r] ? a[r] : minb[r];
        if (den > 0.0) s = (minb[r] - a[r]) / den;
      }
      p.sil[p.v.perm[pos]] = s;
    }
  }
}

// compensated sum of x[0 .. cnt) by one workgroup: strided per thread, then a fixed tree in LDS; the total in every thread
template <int NT>
__device__ __forceinline__ double cq_block_sum(const double *x, int64_t cnt, double *sh) {
  double s = 0.0, c = 0.0;
  for (int64_t i = threadIdx.x; i < cnt; i += NT) {
    const double y = x[i] - c, z = s + y;
    c = (z - s) - y;
    s = z;
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = NT / 2; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  return sh[0];
}

__global__ __launch_bounds__(1024) void k_cq_mean(const double *sil, int n, double *mean) {
  __shared__ double sh[1024];
  const double s = cq_block_sum<1024>(sil, n, sh);
  if (threadIdx.x == 0) *mean = s / (double)n;
}

struct CqCoh {
  CqView v;
  const double *nrm2;   // [n] by position
  const int *tiles;     // [n_tiles][3]: cluster, tile row, tile column (row <= column), tiles of a cluster together
  const int *cstart;    // [n_clusters] first position
  const int *csize;     // [n_clusters]
  const double *mean;   // [n_clusters] pass 1: the finished mean
  double *partial;      // [n_tiles]
  int pass;             // 0: sum of c_ij, 1: sum of (c_ij - mean)^2
};

// One 64 x 64 tile of one cluster's pairs i < j, cluster-local coordinates: c_ij = 1 - cos as scipy forms it (the cosine
// clipped to [-1, 1], NaN where a norm is zero).  The tile's sum: per lane in register order, a xor butterfly over the wave,
// the four waves in order.
__global__ __launch_bounds__(kCqNT) void k_cq_cohesion(CqCoh p) {
  __shared__ float As[kCqTile][kCqLd], Bs[kCqTile][kCqLd];
  __shared__ int64_t ra[kCqTile], rb[kCqTile];
  __shared__ double na[kCqTile], nb[kCqTile], ws[kCqNT / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = p.tiles[3 * blockIdx.x], bi = p.tiles[3 * blockIdx.x + 1], bj = p.tiles[3 * blockIdx.x + 2];
  const int st = p.cstart[c], m = p.csize[c];
  if (tid < kCqTile) {
    const int ia = bi * kCqTile + tid, ib = bj * kCqTile + tid;
    ra[tid] = ia < m ? (int64_t)p.v.perm[st + ia] : -1;
    rb[tid] = ib < m ? (int64_t)p.v.perm[st + ib] : -1;
    na[tid] = ia < m ? sqrt(p.nrm2[st + ia]) : 0.0;
    nb[tid] = ib < m ? sqrt(p.nrm2[st + ib]) : 0.0;
  }
  __syncthreads();
  double4_t acc[4];
  cq_tile_gram(p.v.x32, p.v.dim, ra, rb, As, Bs, acc);
  const double mu = p.pass ? p.mean[c] : 0.0;
  double s = 0.0;
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int li = w * 16 + (lane >> 4) + 4 * r, lj = b * 16 + (lane & 15);
      const int i = bi * kCqTile + li, j = bj * kCqTile + lj;
      if (i < j && j < m) {
        double cosv = acc[b][r] / (na[li] * nb[lj]);
        if (fabs(cosv) > 1.0) cosv = copysign(1.0, cosv);
        const double cd = 1.0 - cosv;
        s += p.pass ? (cd - mu) * (cd - mu) : cd;
      }
    }
  for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o);
  if (lane == 0) ws[w] = s;
  __syncthreads();
  if (tid == 0) p.partial[blockIdx.x] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

// a cluster's tiles summed in one fixed order; pass 0 -> mean, pass 1 -> population standard deviation
__global__ __launch_bounds__(kCqNT) void k_cq_coh_reduce(const double *partial, const int64_t *toff, const int *csize, int pass,
                                                         double *mean, double *sd) {
  __shared__ double sh[kCqNT];
  const int c = blockIdx.x;
  const double s = cq_block_sum<kCqNT>(partial + toff[c], toff[c + 1] - toff[c], sh);
  if (threadIdx.x == 0) {
    const double m = (double)csize[c], pairs = m * (m - 1.0) / 2.0;
    if (pass == 0) mean[c] = s / pairs;
    else sd[c] = sqrt(s / pairs);
  }
}

// developer timing (anr_cluster_quality_timing): HIP-event times of the last timed call
bool g_timing = false;
float g_times[3] = {0.f, 0.f, 0.f};  // silhouette group, cohesion group, first copy in to last copy out

}  // namespace

extern "C" int anr_cluster_quality_timing(int32_t enable, float *ms3) {
  g_timing = enable != 0;
  if (ms3) std::copy(g_times, g_times + 3, ms3);
  return ANR_OK;
}

extern "C" int anr_index_cluster_quality(anr_index *h, const int32_t *labels_host, double *sil_samples, double *sil_mean,
                                         int64_t label_cap, int32_t *labels_out, int64_t *sizes, double *cohesion,
                                         double *cohesion_std, int64_t *n_labels, int64_t *stats) {
  if (!h) return fail(ANR_EINVAL, "null handle");
  const IndexCore c0 = index_core(h);
  if (c0.metric != ANR_METRIC_L2 || c0.normalize)
    return fail(ANR_EINVAL, "cluster quality needs an L2 index that stores its rows as given (no normalisation)");
  DeviceGuard g(c0.device);
  if (!g.ok) return fail(ANR_EHIP, "hipSetDevice(%d) failed", c0.device);
  std::lock_guard<std::mutex> lk(*c0.mu);
  const IndexCore cur = index_core(h);  // under the lock: an add may have moved the rows
  if (cur.ntotal == 0) return ANR_OK;
  if (!labels_host) return fail(ANR_EINVAL, "cluster quality: null labels");
  if (cur.ntotal > (int64_t)INT_MAX - kCqTile) return fail(ANR_EINVAL, "cluster quality: too many rows for one call");
  const int n = (int)cur.ntotal;

  // the label runs of the sorted order, on the host: distinct labels ascending and their sizes
  std::vector<int32_t> sorted(labels_host, labels_host + n);
  std::sort(sorted.begin(), sorted.end());
  std::vector<int32_t> seg_label;
  std::vector<int> seg_start, segpos((size_t)n);
  for (int i = 0; i < n; ++i) {
    if (i == 0 || sorted[i] != sorted[i - 1]) {
      seg_label.push_back(sorted[i]);
      seg_start.push_back(i);
    }
    segpos[i] = (int)seg_label.size() - 1;
  }
  seg_start.push_back(n);
  const int64_t nl = (int64_t)seg_label.size();
  const bool per_label = labels_out || sizes || cohesion || cohesion_std;
  if (per_label && label_cap < nl) {
    if (n_labels) *n_labels = nl;
    return fail(ANR_EINVAL, "cluster quality: %lld distinct labels, room for %lld", (long long)nl, (long long)label_cap);
  }
  const bool want_sil = sil_samples || sil_mean, want_coh = cohesion || cohesion_std;

  // clusters with a cohesion (label >= 0, two rows or more) and their tiles
  std::vector<int> cseg, cstart, csize, tiles;
  std::vector<int64_t> toff(1, 0);
  if (want_coh)
    for (int64_t s = 0; s < nl; ++s) {
      const int m = seg_start[s + 1] - seg_start[s];
      if (seg_label[s] < 0 || m < 2) continue;
      const int ci = (int)cseg.size(), nb = (int)ceil_div(m, kCqTile);
      cseg.push_back((int)s);
      cstart.push_back(seg_start[s]);
      csize.push_back(m);
      for (int bi = 0; bi < nb; ++bi)
        for (int bj = bi; bj < nb; ++bj) {
          tiles.push_back(ci);
          tiles.push_back(bi);
          tiles.push_back(bj);
        }
      toff.push_back((int64_t)tiles.size() / 3);
    }
  const int64_t nc = (int64_t)cseg.size(), n_tiles = (int64_t)tiles.size() / 3;
  if (n_tiles > 0x7fffffffLL) return fail(ANR_EINVAL, "cluster quality: too many cluster tiles for one launch");

  // arena: inputs (one copy in), work arrays, outputs (one copy back)
  ArenaLayout<256> L;
  const size_t o_labels = L.take((size_t)n * 4), o_segpos = L.take((size_t)n * 4), o_segstart = L.take((size_t)(nl + 1) * 4);
  const size_t o_cstart = L.take((size_t)nc * 4), o_csize = L.take((size_t)nc * 4), o_toff = L.take((size_t)(nc + 1) * 8);
  const size_t o_tiles = L.take(tiles.size() * 4), in_end = L.at;
  const size_t o_kin = L.take((size_t)n * 8), o_kout = L.take((size_t)n * 8), o_iota = L.take((size_t)n * 4);
  const size_t o_perm = L.take((size_t)n * 4), o_nrm2 = L.take((size_t)n * 8), o_partial = L.take((size_t)n_tiles * 8);
  const size_t o_sort = L.take(radix_sort_temp_bytes(n));
  const size_t o_out = L.at;
  const size_t o_sil = L.take((size_t)n * 8), o_mean = L.take(8), o_cmean = L.take((size_t)nc * 8);
  const size_t o_csd = L.take((size_t)nc * 8);
  const size_t out_end = L.at;

  DevBuf<unsigned char> &arena = index_scratch(h).cq_arena;
  ANR_TRY(arena.alloc((int64_t)out_end, "cluster quality", (int64_t)(out_end + out_end / 4)));
  unsigned char *A = arena.p;
  hipStream_t st = cur.stream;

  std::vector<unsigned char> in(in_end, 0);
  memcpy(&in[o_labels], labels_host, (size_t)n * 4);
  memcpy(&in[o_segpos], segpos.data(), (size_t)n * 4);
  memcpy(&in[o_segstart], seg_start.data(), (size_t)(nl + 1) * 4);
  if (nc) {
    memcpy(&in[o_cstart], cstart.data(), (size_t)nc * 4);
    memcpy(&in[o_csize], csize.data(), (size_t)nc * 4);
    memcpy(&in[o_tiles], tiles.data(), tiles.size() * 4);
  }
  memcpy(&in[o_toff], toff.data(), (size_t)(nc + 1) * 8);

  Events<4> ev;
  if (g_timing) ANR_TRY(ev.init());
  ANR_TRY(ev.mark(0, st));
  ANR_HIP(hipMemcpyAsync(A, in.data(), in_end, hipMemcpyHostToDevice, st));
  ANR_HIP(hipMemsetAsync(A + o_out, 0, out_end - o_out, st));

  // sorted order and the diagonal of G
  unsigned *perm = reinterpret_cast<unsigned *>(A + o_perm);
  double *nrm2 = reinterpret_cast<double *>(A + o_nrm2);
  const unsigned g256 = (unsigned)ceil_div(n, 256), strips = (unsigned)ceil_div(n, kCqTile);
  hipLaunchKernelGGL(k_cq_keys, dim3(g256), dim3(256), 0, st, reinterpret_cast<const int *>(A + o_labels), n,
                     reinterpret_cast<unsigned long long *>(A + o_kin), reinterpret_cast<unsigned *>(A + o_iota));
  ANR_HIP(hipGetLastError());
  ANR_TRY(radix_sort_pairs_u64(A + o_sort, reinterpret_cast<const unsigned long long *>(A + o_kin),
                               reinterpret_cast<unsigned long long *>(A + o_kout),
                               reinterpret_cast<const unsigned *>(A + o_iota), perm, n, false, st));
  const CqView v{cur.x32, cur.dim, n, perm};
  hipLaunchKernelGGL(k_cq_norms, dim3(strips), dim3(kCqNT), 0, st, v, nrm2);
  ANR_HIP(hipGetLastError());

  if (want_sil) {
    const CqSil sp{v, reinterpret_cast<const int *>(A + o_segpos), reinterpret_cast<const int *>(A + o_segstart), nrm2,
                   reinterpret_cast<double *>(A + o_sil)};
    hipLaunchKernelGGL(k_cq_silhouette, dim3(strips), dim3(kCqNT), 0, st, sp);
    ANR_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_cq_mean, dim3(1), dim3(1024), 0, st, sp.sil, n, reinterpret_cast<double *>(A + o_mean));
    ANR_HIP(hipGetLastError());
  }
  ANR_TRY(ev.mark(1, st));
  if (n_tiles > 0) {
    CqCoh cp{v,
             nrm2,
             reinterpret_cast<const int *>(A + o_tiles),
             reinterpret_cast<const int *>(A + o_cstart),
             reinterpret_cast<const int *>(A + o_csize),
             reinterpret_cast<const double *>(A + o_cmean),
             reinterpret_cast<double *>(A + o_partial),
             0};
    for (int pass = 0; pass < 2; ++pass) {  // the deviations are taken against the finished mean: a second walk
      cp.pass = pass;
      hipLaunchKernelGGL(k_cq_cohesion, dim3((unsigned)n_tiles), dim3(kCqNT), 0, st, cp);
      ANR_HIP(hipGetLastError());
      hipLaunchKernelGGL(k_cq_coh_reduce, dim3((unsigned)nc), dim3(kCqNT), 0, st, cp.partial,
                         reinterpret_cast<const int64_t *>(A + o_toff), cp.csize, pass,
                         reinterpret_cast<double *>(A + o_cmean), reinterpret_cast<double *>(A + o_csd));
      ANR_HIP(hipGetLastError());
    }
  }
  ANR_TRY(ev.mark(2, st));
  std::vector<unsigned char> out(out_end - o_out);
  ANR_HIP(hipMemcpyAsync(out.data(), A + o_out, out.size(), hipMemcpyDeviceToHost, st));
  ANR_TRY(ev.mark(3, st));
  ANR_HIP(hipStreamSynchronize(st));
  if (ev.on) {
    ANR_TRY(ev.elapsed(0, 1, &g_times[0]));
    ANR_TRY(ev.elapsed(1, 2, &g_times[1]));
    ANR_TRY(ev.elapsed(0, 3, &g_times[2]));
  }
  const unsigned char *O = out.data() - o_out;
  if (sil_samples) memcpy(sil_samples, O + o_sil, (size_t)n * 8);
  if (sil_mean) memcpy(sil_mean, O + o_mean, 8);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int64_t s = 0; s < nl; ++s) {
    if (labels_out) labels_out[s] = seg_label[s];
    if (sizes) sizes[s] = seg_start[s + 1] - seg_start[s];
    if (cohesion) cohesion[s] = nan;
    if (cohesion_std) cohesion_std[s] = nan;
  }
  for (int64_t ci = 0; ci < nc; ++ci) {
    if (cohesion) cohesion[cseg[ci]] = reinterpret_cast<const double *>(O + o_cmean)[ci];
    if (cohesion_std) cohesion_std[cseg[ci]] = reinterpret_cast<const double *>(O + o_csd)[ci];
  }
  if (n_labels) *n_labels = nl;
  if (stats) {
    std::fill(stats, stats + 8, (int64_t)0);
    stats[0] = nl;
    for (int64_t s = 0; s < nl; ++s)
      if (seg_label[s] == -1) stats[1] = seg_start[s + 1] - seg_start[s];
    stats[2] = want_sil ? (int64_t)strips * strips : 0;
    stats[3] = n_tiles;
    stats[4] = nc;
    stats[5] = arena.cap;
    stats[6] = (int64_t)ceil_div(cur.dim, kGramKC) * (kGramKC / 4);
  }
  return ANR_OK;
}
