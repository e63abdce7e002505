// anr_index_hdbscan_mst and anr_hdbscan_labels (include/anorag.h): the default branch of the reference's
// TopicClustering._cpu_clustering, sklearn's HDBSCAN(min_cluster_size, min_samples, metric='euclidean',
// cluster_selection_epsilon) (doc/clustering.py:73-79, :99), on the stored float32 rows of an L2 index that does not
// normalise.  The two O(N^2 d) passes run here: the core distances (k_hd_core) and the N - 1 steps of Prim's algorithm over
// the mutual-reachability distance (k_hd_prim, one launch per step, no host synchronisation between them).  The tree stage
// that follows is host work (hdbscan_tree.hpp).  Everything is sklearn's float64 arithmetic bit for bit: one distance
// function (hd_step, then a correctly rounded square root), compared as rounded roots, never as squares; ties go to the lowest
// row; no floating-point atomics.  DESIGN.md §5l has the kernels and the orders, tests/hdbscan_ref.py restates them in numpy.
// Compiled without multiply-add contraction (Makefile, EXACT).
#include <climits>
#include <cmath>
#include <mutex>
#include <vector>

#include "common.hpp"
#include "graph.hpp"
#include "hdbscan_tree.hpp"

using namespace anr;

namespace {

constexpr int kHdMaxMinSamples = 16;  // HDBSCAN_MAX_MIN_SAMPLES: the values a core-distance thread keeps per row
constexpr int kHdTile = 64;           // k_hd_core: rows of a workgroup, and rows of one swept chunk
constexpr int kHdKC = 32;             // dimensions staged through LDS at a time
constexpr int kHdLd = kHdKC + 1;      // floats per LDS row: lane * 33 + k walks all 32 banks
constexpr int kHdNT = 256;            // k_hd_core: 16 x 16 threads, 4 x 4 accumulators each
constexpr int kHdPrimRows = 128;      // k_hd_prim: rows (= lanes) of a workgroup
constexpr unsigned long long kHdNoKey = ~0ull;

// The one distance step: sklearn's float64 (x_k - y_k) * (x_k - y_k) added to the running sum, three roundings.
__device__ __forceinline__ double hd_step(double acc, float a, float b) {
  const double t = (double)a - (double)b;
  return acc + t * t;
}

// keep the KEEP smallest values seen, ascending; every index is a constant, so the list stays in registers
template <int KEEP>
__device__ __forceinline__ void hd_insert(double (&best)[KEEP], double v) {
#pragma unroll
  for (int q = KEEP - 1; q > 0; --q) best[q] = v < best[q - 1] ? best[q - 1] : (v < best[q] ? v : best[q]);
  best[0] = v < best[0] ? v : best[0];
}

// core[i] = the min_samples-th smallest distance of row i to all rows, itself included.  A workgroup owns 64 rows and
// sweeps all rows in chunks of 64; both blocks go through LDS as float32, 32 dimensions at a time.  Thread (ti, tj) holds
// the 4 x 4 sums of rows 4 ti .. 4 ti + 3 against chunk rows tj, tj + 16, tj + 32, tj + 48, each summed in ascending k
// (dimensions beyond dim are staged as zeros: + 0.0 changes no sum).  It keeps the KEEP >= min_samples smallest distances
// of its four rows; the 16 threads of a row are 16 neighbouring lanes and merge their lists by a xor butterfly.  Only
// values matter, so equal distances need no order.
template <int KEEP>
__global__ __launch_bounds__(kHdNT) void k_hd_core(const float *__restrict__ x, int n, int dim, int min_samples,
                                                   double *__restrict__ core) {
  __shared__ float As[kHdTile][kHdLd];
  __shared__ float Bs[kHdTile][kHdLd];
  const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
  const int i0 = blockIdx.x * kHdTile;
  double best[4][KEEP];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int q = 0; q < KEEP; ++q) best[r][q] = INFINITY;
  for (int j0 = 0; j0 < n; j0 += kHdTile) {
    double acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
    for (int k0 = 0; k0 < dim; k0 += kHdKC) {
      __syncthreads();  // the previous block of dimensions has been consumed
      for (int e = tid; e < kHdTile * kHdKC; e += kHdNT) {
        const int r = e / kHdKC, k = e % kHdKC, kk = k0 + k;
        As[r][k] = (i0 + r < n && kk < dim) ? x[(int64_t)(i0 + r) * dim + kk] : 0.f;
        Bs[r][k] = (j0 + r < n && kk < dim) ? x[(int64_t)(j0 + r) * dim + kk] : 0.f;
      }
      __syncthreads();
#pragma unroll 8
      for (int k = 0; k < kHdKC; ++k) {
        float a[4], b[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) a[r] = As[ti * 4 + r][k];
#pragma unroll
        for (int c = 0; c < 4; ++c) b[c] = Bs[tj + 16 * c][k];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[r][c] = hd_step(acc[r][c], a[r], b[c]);
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (j0 + tj + 16 * c < n) {
#pragma unroll
        for (int r = 0; r < 4; ++r) hd_insert<KEEP>(best[r], __dsqrt_rn(acc[r][c]));
      }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      double mine[KEEP];
#pragma unroll
      for (int q = 0; q < KEEP; ++q) mine[q] = best[r][q];
#pragma unroll
      for (int q = 0; q < KEEP; ++q) hd_insert<KEEP>(best[r], __shfl_xor(mine[q], o));
    }
    double kth = 0.0;
#pragma unroll
    for (int q = 0; q < KEEP; ++q)
      if (q == min_samples - 1) kth = best[r][q];
    const int row = i0 + ti * 4 + r;
    if (tj == 0 && row < n) core[row] = kth;
  }
}

// the state of Prim's algorithm between its steps
struct HdPrim {
  const float *x;
  int n, dim;
  const double *core;
  double *reach;             // [n] min_reachability
  int *source;               // [n] the tree row that gave reach[j]
  int *in_tree;              // [n]
  int *cur;                  // the row added last
  unsigned *counter;         // tickets of the step's workgroups, zero between steps
  unsigned long long *pkey;  // [workgroups] a workgroup's smallest reach, as its bit pattern
  int *prow;                 // [workgroups] ... and the row it belongs to
  int *e_src, *e_dst;        // [n - 1] the edges in the order they are added
  double *e_w;
  int *flags;                // [0] a row holds a NaN or an infinity; [1] a step found no row outside the tree
};

// (key, row) pairs in lexicographic order: the smaller distance, and among equal distances the lower row.  Distances are
// non-negative doubles, whose order is the order of their bit patterns.
__device__ __forceinline__ void hd_take_smaller(unsigned long long &key, int &row, unsigned long long okey, int orow) {
  if (okey < key || (okey == key && orow < row)) key = okey, row = orow;
}

// the workgroup's smallest pair, valid in thread 0
__device__ __forceinline__ void hd_block_min(unsigned long long &key, int &row, unsigned long long *skey, int *srow) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long okey = __shfl_xor(key, o);
    const int orow = __shfl_xor(row, o);
    hd_take_smaller(key, row, okey, orow);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) skey[wave] = key, srow[wave] = row;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < kHdPrimRows / 64; ++w) hd_take_smaller(key, row, skey[w], srow[w]);
}

__global__ void k_hd_init(HdPrim p) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < p.n) {
    p.reach[j] = INFINITY;
    p.source[j] = 1;
    p.in_tree[j] = j == 0;
  }
  if (j == 0) *p.cur = 0, *p.counter = 0u, p.flags[0] = 0, p.flags[1] = 0;
}

// flags[0] = 1 if any stored value is a NaN or an infinity (exponent bits all ones); runs after k_hd_init
__global__ void k_hd_finite(HdPrim p) {
  const int64_t total = (int64_t)p.n * p.dim;
  bool bad = false;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x)
    bad |= (__float_as_uint(p.x[e]) & 0x7f800000u) == 0x7f800000u;
  if (bad) atomicOr(p.flags, 1);
}

// Step `step` of Prim's algorithm from the row *cur.  A lane owns row j: 128 rows x 32 dimensions go through LDS at a time
// (read along the rows, consumed down a column), x_cur beside them.  A row outside the tree lowers its reach to
// max(core[cur], core[j], dist) where that is smaller, remembering cur; the workgroup reduces (reach, row) and publishes
// one pair.  The workgroup that draws the step's last ticket reduces the published pairs the same way, writes the edge,
// puts the row into the tree, makes it the next step's cur and zeroes the counter.  Nobody waits for anybody.
__global__ __launch_bounds__(kHdPrimRows) void k_hd_prim(HdPrim p, int step) {
  __shared__ float Xs[kHdPrimRows][kHdLd];
  __shared__ float Cs[kHdKC];
  __shared__ unsigned long long skey[kHdPrimRows / 64];
  __shared__ int srow[kHdPrimRows / 64];
  __shared__ unsigned sticket;
  const int tid = threadIdx.x, j0 = blockIdx.x * kHdPrimRows, j = j0 + tid;
  const int cur = *p.cur;
  double acc = 0.0;
  for (int k0 = 0; k0 < p.dim; k0 += kHdKC) {
    __syncthreads();
    for (int e = tid; e < kHdPrimRows * kHdKC; e += kHdPrimRows) {
      const int r = e / kHdKC, k = e % kHdKC, kk = k0 + k;
      Xs[r][k] = (j0 + r < p.n && kk < p.dim) ? p.x[(int64_t)(j0 + r) * p.dim + kk] : 0.f;
    }
    if (tid < kHdKC) Cs[tid] = k0 + tid < p.dim ? p.x[(int64_t)cur * p.dim + k0 + tid] : 0.f;
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < kHdKC; ++k) acc = hd_step(acc, Cs[k], Xs[tid][k]);
  }
  unsigned long long key = kHdNoKey;
  int row = INT_MAX;
  if (j < p.n && !p.in_tree[j]) {
    const double dist = __dsqrt_rn(acc);
    const double cc = p.core[cur], cj = p.core[j];
    double mr = cc > cj ? cc : cj;
    mr = dist > mr ? dist : mr;
    double have = p.reach[j];
    if (mr < have) {
      have = mr;
      p.reach[j] = mr;
      p.source[j] = cur;
    }
    key = (unsigned long long)__double_as_longlong(have);
    row = j;
  }
  hd_block_min(key, row, skey, srow);
  if (tid == 0) {
    __hip_atomic_store(p.pkey + blockIdx.x, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(p.prow + blockIdx.x, row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sticket = __hip_atomic_fetch_add(p.counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (sticket != gridDim.x - 1) return;
  key = kHdNoKey, row = INT_MAX;
  for (int b = tid; b < (int)gridDim.x; b += kHdPrimRows)
    hd_take_smaller(key, row, __hip_atomic_load(p.pkey + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                    __hip_atomic_load(p.prow + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  __syncthreads();  // skey / srow of the first reduction have been read
  hd_block_min(key, row, skey, srow);
  if (tid == 0) {
    if (row >= p.n) {  // cannot happen on finite rows: the call ends with an error; every later index stays inside the arrays
      p.flags[1] = 1;
      row = 0;
    }
    p.e_src[step] = p.source[row];
    p.e_dst[step] = row;
    p.e_w[step] = __longlong_as_double((long long)key);
    p.in_tree[row] = 1;
    *p.cur = row;
    __hip_atomic_store(p.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <int KEEP>
int launch_core(const IndexCore &c, int n, int min_samples, double *core) {
  hipLaunchKernelGGL(k_hd_core<KEEP>, dim3((unsigned)ceil_div(n, kHdTile)), dim3(kHdNT), 0, c.stream, c.x32, n, c.dim,
                     min_samples, core);
  ANR_HIP(hipGetLastError());
  return ANR_OK;
}

}  // namespace

extern "C" int anr_index_hdbscan_mst(anr_index *h, int32_t min_samples, double *core, int64_t *src, int64_t *dst, double *w,
                                     int64_t *stats) {
  if (!h) return fail(ANR_EINVAL, "null handle");
  const IndexCore c0 = index_core(h);
  if (c0.metric != ANR_METRIC_L2 || c0.normalize)
    return fail(ANR_EINVAL, "hdbscan needs an L2 index that stores its rows as given (no normalisation)");
  DeviceGuard g(c0.device);
  if (!g.ok) return fail(ANR_EHIP, "hipSetDevice(%d) failed", c0.device);
  std::lock_guard<std::mutex> lk(*c0.mu);
  const IndexCore cur = index_core(h);  // under the lock: an add may have moved the rows
  if (cur.ntotal < 2) return fail(ANR_EINVAL, "hdbscan: n_samples = %lld, at least 2 rows are needed", (long long)cur.ntotal);
  if (cur.ntotal > (int64_t)INT_MAX - kHdPrimRows) return fail(ANR_EINVAL, "hdbscan: too many rows for one call");
  if (min_samples < 1) return fail(ANR_EINVAL, "hdbscan: min_samples = %d, at least 1 is needed", min_samples);
  if (min_samples > kHdMaxMinSamples)
    return fail(ANR_EINVAL, "hdbscan: min_samples = %d is above the %d this kernel keeps", min_samples, kHdMaxMinSamples);
  if (min_samples > cur.ntotal)
    return fail(ANR_EINVAL, "hdbscan: min_samples (%d) must be at most the number of samples in X (%lld)", min_samples,
                (long long)cur.ntotal);
  if (!core || !src || !dst || !w) return fail(ANR_EINVAL, "hdbscan: null core, src, dst or w");
  const int n = (int)cur.ntotal;
  const size_t N = (size_t)n, E = N - 1;
  const int nwg = (int)ceil_div(n, kHdPrimRows);

  ArenaLayout<256> L;
  const size_t o_core = L.take(N * 8), o_reach = L.take(N * 8), o_w = L.take(E * 8), o_pkey = L.take((size_t)nwg * 8);
  const size_t o_source = L.take(N * 4), o_tree = L.take(N * 4), o_src = L.take(E * 4), o_dst = L.take(E * 4);
  const size_t o_prow = L.take((size_t)nwg * 4), o_cur = L.take(4), o_counter = L.take(4), o_flags = L.take(8);
  DevBuf<unsigned char> arena;  // of this call: freed on return, after the stream has drained
  ANR_TRY(arena.alloc((int64_t)L.at, "hdbscan"));
  unsigned char *A = arena.p;
  HdPrim p{};
  p.x = cur.x32, p.n = n, p.dim = cur.dim;
  p.core = reinterpret_cast<double *>(A + o_core), p.reach = reinterpret_cast<double *>(A + o_reach);
  p.e_w = reinterpret_cast<double *>(A + o_w), p.pkey = reinterpret_cast<unsigned long long *>(A + o_pkey);
  p.source = reinterpret_cast<int *>(A + o_source), p.in_tree = reinterpret_cast<int *>(A + o_tree);
  p.e_src = reinterpret_cast<int *>(A + o_src), p.e_dst = reinterpret_cast<int *>(A + o_dst);
  p.prow = reinterpret_cast<int *>(A + o_prow), p.cur = reinterpret_cast<int *>(A + o_cur);
  p.counter = reinterpret_cast<unsigned *>(A + o_counter), p.flags = reinterpret_cast<int *>(A + o_flags);
  hipStream_t st = cur.stream;
  Events<3> ev;  // around the two passes, for stats[4] and stats[5]: only when stats are asked for
  if (stats) ANR_TRY(ev.init());
  int flags[2] = {0, 0};

  // on any failure below the stream is drained before the arena goes
  auto run = [&]() -> int {
    hipLaunchKernelGGL(k_hd_init, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, p);
    ANR_HIP(hipGetLastError());
    // the rows must be finite: found out here, on the device, before either pass starts
    const int64_t fin_blocks = std::min<int64_t>(ceil_div((int64_t)n * cur.dim, 256), 4096);
    hipLaunchKernelGGL(k_hd_finite, dim3((unsigned)fin_blocks), dim3(256), 0, st, p);
    ANR_HIP(hipGetLastError());
    ANR_HIP(hipMemcpyAsync(flags, p.flags, sizeof(flags), hipMemcpyDeviceToHost, st));
    ANR_HIP(hipStreamSynchronize(st));
    if (flags[0]) return fail(ANR_EINVAL, "hdbscan: the rows hold NaN or infinite values");
    double *core_dev = reinterpret_cast<double *>(A + o_core);
    ANR_TRY(ev.mark(0, st));
    if (min_samples <= 4) ANR_TRY(launch_core<4>(cur, n, min_samples, core_dev));
    else if (min_samples <= 8) ANR_TRY(launch_core<8>(cur, n, min_samples, core_dev));
    else ANR_TRY(launch_core<16>(cur, n, min_samples, core_dev));
    ANR_TRY(ev.mark(1, st));
    for (int step = 0; step < n - 1; ++step) {
      hipLaunchKernelGGL(k_hd_prim, dim3((unsigned)nwg), dim3(kHdPrimRows), 0, st, p, step);
      ANR_HIP(hipGetLastError());
    }
    return ev.mark(2, st);
  };
  std::vector<int> hs(E), hd(E);
  int rc = run();
  if (rc == ANR_OK) {
    auto copy = [&]() -> int {
      ANR_HIP(hipMemcpyAsync(core, p.core, N * 8, hipMemcpyDeviceToHost, st));
      ANR_HIP(hipMemcpyAsync(w, p.e_w, E * 8, hipMemcpyDeviceToHost, st));
      ANR_HIP(hipMemcpyAsync(hs.data(), p.e_src, E * 4, hipMemcpyDeviceToHost, st));
      ANR_HIP(hipMemcpyAsync(hd.data(), p.e_dst, E * 4, hipMemcpyDeviceToHost, st));
      ANR_HIP(hipMemcpyAsync(flags, p.flags, sizeof(flags), hipMemcpyDeviceToHost, st));
      return ANR_OK;
    };
    rc = copy();
  }
  const hipError_t se = hipStreamSynchronize(st);
  if (rc != ANR_OK) return rc;
  if (se != hipSuccess) return fail(ANR_EHIP, "hdbscan: hipStreamSynchronize failed: %s", hipGetErrorString(se));
  if (flags[1]) return fail(ANR_EINTERNAL, "hdbscan: a Prim step found no row outside the tree");
  for (size_t i = 0; i < E; ++i) src[i] = hs[i], dst[i] = hd[i];
  if (stats) {
    std::fill(stats, stats + 8, (int64_t)0);
    stats[0] = n - 1;
    stats[1] = ceil_div(n, kHdTile) * ceil_div(n, kHdTile);
    stats[2] = arena.cap;
    stats[3] = nwg;
    float ms_core = 0.f, ms_prim = 0.f;  // the times are an extra: where an event cannot be read they stay 0
    if (ev.elapsed(0, 1, &ms_core) == ANR_OK && ev.elapsed(1, 2, &ms_prim) == ANR_OK)
      stats[4] = (int64_t)(ms_core * 1e3f), stats[5] = (int64_t)(ms_prim * 1e3f);
  }
  return ANR_OK;
}

extern "C" int anr_hdbscan_labels(int64_t n, const int64_t *src, const int64_t *dst, const double *w, int32_t min_cluster_size,
                                  double eps, int32_t *labels, int64_t *stats) {
  std::string err;
  if (hdbscan_labels_host(n, src, dst, w, min_cluster_size, eps, labels, stats, &err) != 0)
    return fail(ANR_EINVAL, "%s", err.c_str());
  return ANR_OK;
}
