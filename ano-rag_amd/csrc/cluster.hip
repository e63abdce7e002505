// anr_index_dbscan (include/anorag.h): DBSCAN topic clustering over the stored rows of a flat index — the device producer
// for the `dbscan` branch of the reference's TopicClustering._cpu_clustering (doc/clustering.py:88-99), which
// DocumentProcessor.process_documents reaches on every build (doc/document_processor.py:181).  Host orchestration of the
// kernels in cluster_kernels.hpp; DESIGN.md §5f has the closed form, the error band and the measurements.
#include <algorithm>
#include <cmath>
#include <mutex>

#include "cluster.hpp"
#include "cluster_kernels.hpp"
#include "common.hpp"
#include "graph.hpp"

using namespace anr;

namespace {

template <int PASS>
int launch_walk(const DbscanWalk &w, int n_cu, hipStream_t st) {
  constexpr int slots_bytes = 2 * 4 * 16 * 1024;
  ANR_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(&k_dbscan_walk<PASS>), slots_bytes));
  const int64_t persistent = std::min<int64_t>(w.n_slots, std::max(8, n_cu / 8 * 8));  // a multiple of 8: slot % 8 = XCD
  hipLaunchKernelGGL(k_dbscan_walk<PASS>, dim3((unsigned)persistent), dim3(512), slots_bytes, st, w);
  ANR_HIP(hipGetLastError());
  return ANR_OK;
}

// a float32 above / below the value, so that rounding the thresholds never narrows the band
float f32_above(double v) {
  const float f = (float)v;
  return std::isfinite(f) ? std::nextafterf(std::nextafterf(f, INFINITY), INFINITY) : f;
}
float f32_below(double v) {
  const float f = (float)v;
  return std::isfinite(f) ? std::nextafterf(std::nextafterf(f, -INFINITY), -INFINITY) : f;
}

}  // namespace

extern "C" int anr_index_dbscan(anr_index *h, double eps, int32_t min_samples, int32_t *labels_host, int64_t *stats) {
  if (!h) return fail(ANR_EINVAL, "null handle");
  if (!(eps == eps) || eps < 0.0) return fail(ANR_EINVAL, "eps must be a number >= 0");
  if (min_samples < 1) return fail(ANR_EINVAL, "min_samples must be >= 1");
  const IndexCore c = index_core(h);
  if (c.metric == ANR_METRIC_IP && !c.normalize)
    return fail(ANR_EINVAL, "dbscan needs an L2 index or a normalising inner-product index (cosine distance)");
  DeviceGuard g(c.device);
  if (!g.ok) return fail(ANR_EHIP, "hipSetDevice(%d) failed", c.device);
  std::lock_guard<std::mutex> lk(*c.mu);
  JoinView v{};
  ANR_TRY(index_join_view(h, &v));
  if (stats) std::fill(stats, stats + 8, (int64_t)0);
  const int64_t n = v.ntotal;
  if (n == 0) return ANR_OK;
  if (!labels_host) return fail(ANR_EINVAL, "null labels");
  if (v.f16_unusable) return fail(ANR_ESTATE, "stored values exceed the f16 range: the f16 image cannot decide pairs");
  const bool l2 = v.metric == ANR_METRIC_L2;

  // |x16_i . x16_j - x_i . x_j| <= |x_i||dx_j| + |dx_i||x16_j| (+ f32 accumulation of the MFMA), as in the self join.  The
  // kernel compares w = x16_i . x16_j (+ b_i + b_j, b = -||x||^2 / 2 as stored): w is 1 - D on a cosine index, -D^2 / 2 on
  // an L2 index — in D (cosine) or D^2 (L2) the band is twice this one.  L2 adds the rounding of the two stored squared
  // norms (dimp / 8 + 8 float32 additions each) and of the two additions that form w.
  const double xmax = v.xmax, xerr = v.xerr;
  double band = 2.0 * xmax * xerr + xerr * xerr + 2.0 * v.dimp * 5.9604645e-8 * xmax * xmax;
  if (l2) band += (v.dimp / 8 + 32) * 5.9604645e-8 * xmax * xmax;
  const double thr = l2 ? -0.5 * eps * eps : 1.0 - eps;
  band += 1e-7 * (std::fabs(thr) + 1.0);

  const int64_t n_tiles = ceil_div(n, kTileRows);
  const int nblk = (int)ceil_div(n_tiles, 8);
  const PatchGrid pg = make_patch_grid(nblk, nblk);
  if (pg.grid() > 0x7fffffffLL) return fail(ANR_EINVAL, "too many rows for one dbscan launch");

  hipStream_t st = v.stream;
  DevBuf<unsigned> count, parent, border, rank, blk;  // buffers of this call
  DevBuf<int> labels;
  DevBuf<unsigned long long> counters;
  DevBuf<uint2> cand, inpairs;
  ANR_TRY(count.alloc(n, "dbscan"));
  ANR_TRY(parent.alloc(n, "dbscan"));
  ANR_TRY(border.alloc(n, "dbscan"));
  ANR_TRY(rank.alloc(n, "dbscan"));
  ANR_TRY(labels.alloc(n, "dbscan"));
  ANR_TRY(blk.alloc(nblk, "dbscan"));
  ANR_TRY(counters.alloc(kDbCounters, "dbscan"));
  unsigned long long hc[kDbCounters] = {};

  DbscanWalk w{};
  w.x16 = v.x16;
  w.rowbias = v.rowbias;
  w.kb = v.kb;
  w.n_rows = n;
  w.n_tiles = n_tiles;
  w.pg = pg;
  w.n_slots = pg.grid();
  w.thr_hi = f32_above(thr + band);
  w.thr_lo = f32_below(thr - band);
  w.count = count.p;
  w.blk = blk.p;
  w.parent = parent.p;
  w.border = border.p;
  w.counters = counters.p;

  // degree pass; the undecided pairs go to a list that is grown to what the pass reports if it was too short
  int64_t walks = 0, retries = 0;
  int64_t cap = std::max<int64_t>(4 * n, 1 << 16);
  for (;;) {
    ANR_TRY(cand.alloc(cap, "dbscan"));
    w.cand = cand.p;
    w.cap = (unsigned long long)cap;
    ANR_HIP(hipMemsetAsync(count.p, 0, (size_t)n * 4, st));
    ANR_HIP(hipMemsetAsync(counters.p, 0, kDbCounters * 8, st));
    ANR_TRY(launch_walk<kDbDegree>(w, v.n_cu, st));
    ++walks;
    ANR_HIP(hipMemcpyAsync(hc, counters.p, sizeof hc, hipMemcpyDeviceToHost, st));
    ANR_HIP(hipStreamSynchronize(st));
    if (hc[kDbCand] <= (unsigned long long)cap) break;
    if (++retries > 2) return fail(ANR_EHIP, "dbscan: the list of undecided pairs kept overflowing");
    cap = (int64_t)hc[kDbCand];
  }
  const unsigned long long n_unc = hc[kDbCand];

  DbscanRows r{};
  r.n = n;
  r.min_samples = min_samples;
  r.count = count.p;
  r.blk = blk.p;
  r.parent = parent.p;
  r.border = border.p;
  r.rank = rank.p;
  r.labels = labels.p;
  r.counters = counters.p;
  const unsigned list_grid = (unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div((int64_t)n_unc, 256), 1), (int64_t)v.n_cu * 16);
  if (n_unc > 0) {
    ANR_TRY(inpairs.alloc((int64_t)n_unc, "dbscan"));
    DbscanResolve rp{v.x32, v.dim, l2 ? 1 : 0, cand.p, n_unc, eps, count.p, inpairs.p,
                     counters.p};
    hipLaunchKernelGGL(k_dbscan_resolve, dim3(list_grid), dim3(256), 0, st, rp);
    ANR_HIP(hipGetLastError());
    ANR_HIP(hipMemcpyAsync(hc, counters.p, sizeof hc, hipMemcpyDeviceToHost, st));
    ANR_HIP(hipStreamSynchronize(st));
    cand.release();
    r.in_pairs = inpairs.p;
    r.n_pairs = hc[kDbResolvedIn];
  }

  // core flags, then the union pass over the same tiles and the resolved pairs
  hipLaunchKernelGGL(k_dbscan_core, dim3((unsigned)nblk), dim3(256), 0, st, r);
  ANR_HIP(hipGetLastError());
  ANR_TRY(launch_walk<kDbUnion>(w, v.n_cu, st));
  ++walks;
  if (r.n_pairs > 0) {
    hipLaunchKernelGGL(k_dbscan_list_union, dim3(list_grid), dim3(256), 0, st, r);
    ANR_HIP(hipGetLastError());
  }
  // pointer jumping to the fixpoint: a round halves every path, so 64 rounds are more than any forest needs
  int64_t rounds = 0;
  for (; rounds < 64;) {
    ANR_HIP(hipMemsetAsync(counters.p + kDbChanged, 0, 8, st));
    hipLaunchKernelGGL(k_dbscan_jump, dim3((unsigned)nblk), dim3(256), 0, st, r);
    ANR_HIP(hipGetLastError());
    ++rounds;
    unsigned long long changed = 0;
    ANR_HIP(hipMemcpyAsync(&changed, counters.p + kDbChanged, 8, hipMemcpyDeviceToHost, st));
    ANR_HIP(hipStreamSynchronize(st));
    if (!changed) break;
    if (rounds == 64) return fail(ANR_EHIP, "dbscan: pointer jumping did not converge");
  }
  // border pass: a third walk, over the block pairs that hold a core row on one side and a row that is not core on the other
  ANR_TRY(launch_walk<kDbBorder>(w, v.n_cu, st));
  ++walks;
  if (r.n_pairs > 0) {
    hipLaunchKernelGGL(k_dbscan_list_border, dim3(list_grid), dim3(256), 0, st, r);
    ANR_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_dbscan_rank, dim3(1), dim3(1024), 0, st, r);
  ANR_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_dbscan_labels, dim3((unsigned)nblk), dim3(256), 0, st, r);
  ANR_HIP(hipGetLastError());
  ANR_HIP(hipMemcpyAsync(hc, counters.p, sizeof hc, hipMemcpyDeviceToHost, st));
  ANR_HIP(hipMemcpyAsync(labels_host, labels.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  ANR_HIP(hipStreamSynchronize(st));
  if (stats) {
    stats[0] = (int64_t)hc[kDbClusters];
    stats[1] = (int64_t)hc[kDbCore];
    stats[2] = (int64_t)hc[kDbNoise];
    stats[3] = (int64_t)n_unc;
    stats[4] = walks;
    stats[5] = rounds;
    stats[6] = retries;
    stats[7] = (int64_t)r.n_pairs;
  }
  return ANR_OK;
}
