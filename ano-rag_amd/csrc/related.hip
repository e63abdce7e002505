// anr_index_related_notes (include/anorag.h): the related notes of every stored row of a cosine index — the device form of
// NoteSimilarityCalculator.find_related_notes (utils/note_similarity.py:115-233), which EnhancedAtomicNoteGenerator runs on
// every note build (llm/enhanced_atomic_note_generator.py:346).  Host orchestration of the kernels in related_kernels.hpp;
// DESIGN.md §5m has the semantics, the error band and the strip passes.
#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>

#include "cluster.hpp"
#include "common.hpp"
#include "graph.hpp"
#include "related_kernels.hpp"

using namespace anr;

namespace {

int64_t g_pair_cap = 0;  // ANR_RELATED_OPT_PAIR_CAP (0: 64 pairs a row, within a quarter of the free device memory)
bool g_timing = false;
float g_times[3] = {0.f, 0.f, 0.f};  // walks, scoring, sort and selection

// device bytes that grow with the pair capacity: the pair, its two records, and the sort's buffers for those
constexpr int64_t kBytesPerPair = 8 + 2 * (8 + 4 + 4 + 4 + 4 + 8 + 8) + 2 * (8 + 4) + 2 * (2 * 8 + 2 * 4);

// a float32 below the value, so that rounding the threshold never narrows the band
float f32_below(double v) {
  const float f = (float)v;
  return std::isfinite(f) ? std::nextafterf(std::nextafterf(f, -INFINITY), -INFINITY) : f;
}

}  // namespace

extern "C" int anr_related_set_option(int32_t option, int64_t value) {
  if (option != ANR_RELATED_OPT_PAIR_CAP) return fail(ANR_EINVAL, "unknown related-notes option %d", option);
  if (value < 0) return fail(ANR_EINVAL, "the pair capacity must be >= 0 (0 = default)");
  g_pair_cap = value;
  return ANR_OK;
}

extern "C" int anr_related_timing(int32_t enable, float *ms3) {
  g_timing = enable != 0;
  if (ms3) std::copy(g_times, g_times + 3, ms3);
  return ANR_OK;
}

extern "C" int anr_index_related_notes(anr_index *h, const anr_related_params *p, const int32_t *cluster,
                                       const int64_t *ent_indptr, const int32_t *ent_ids, int32_t *nbr_host,
                                       int32_t *n_nbr_host, double *comb_host, double *base_host, int32_t *inter_host,
                                       int32_t *uni_host, int64_t *stats) {
  if (!h) return fail(ANR_EINVAL, "null handle");
  if (!p) return fail(ANR_EINVAL, "null parameters");
  const int M = p->max_related;
  if (M < 1 || M > 64) return fail(ANR_EINVAL, "max_related must be in [1, 64], got %d", M);
  const double thr = p->threshold, w = p->entity_weight, bonus = p->cluster_bonus;
  if (!(thr == thr) || !(w == w) || !(bonus == bonus)) return fail(ANR_EINVAL, "a related-notes parameter is NaN");
  const IndexCore c = index_core(h);
  if (c.metric != ANR_METRIC_IP || !c.normalize)
    return fail(ANR_EINVAL, "related notes need a normalising inner-product index (cosine)");
  DeviceGuard g(c.device);
  if (!g.ok) return fail(ANR_EHIP, "hipSetDevice(%d) failed", c.device);
  std::lock_guard<std::mutex> lk(*c.mu);
  JoinView v{};
  ANR_TRY(index_join_view(h, &v));
  if (stats) std::fill(stats, stats + 8, (int64_t)0);
  const int64_t n = v.ntotal;
  if (n == 0) return ANR_OK;
  if (n >= (1ll << 30)) return fail(ANR_EINVAL, "too many rows for related notes");
  if (!nbr_host || !n_nbr_host) return fail(ANR_EINVAL, "null result arrays");
  if (!ent_indptr) return fail(ANR_EINVAL, "null entity rows");
  if (v.f16_unusable) return fail(ANR_ESTATE, "stored values exceed the f16 range: the f16 image cannot nominate pairs");
  if (ent_indptr[0] != 0) return fail(ANR_EINVAL, "ent_indptr must start at 0");
  for (int64_t i = 0; i < n; ++i) {
    if (ent_indptr[i + 1] < ent_indptr[i]) return fail(ANR_EINVAL, "ent_indptr descends at row %lld", (long long)i);
    for (int64_t k = ent_indptr[i]; k < ent_indptr[i + 1]; ++k) {
      if (ent_ids[k] < 0) return fail(ANR_EINVAL, "entity id %d of row %lld is negative", ent_ids[k], (long long)i);
      if (k > ent_indptr[i] && ent_ids[k] <= ent_ids[k - 1])
        return fail(ANR_EINVAL, "the entity ids of row %lld are not strictly ascending", (long long)i);
    }
  }
  const int64_t nnz = ent_indptr[n];
  const int excl = p->exclude_same_cluster != 0;

  // The smallest base that can still pass: base (1 - w) + ent w + cb > thr with ent in [0, 1] and cb <= bonus (only when
  // same-cluster pairs are not excluded).  With 1 - w <= 0 a smaller base never hurts: every pair is a candidate.
  const double one_minus_w = 1.0 - w;
  double base_min = -INFINITY;
  if (one_minus_w > 0.0) base_min = (thr - std::max(w, 0.0) - (excl ? 0.0 : std::max(bonus, 0.0))) / one_minus_w;
  // |x16_i . x16_j - x_i . x_j| <= |x_i||dx_j| + |dx_i||x16_j| (+ f32 accumulation of the MFMA), as in the DBSCAN walk
  const double xmax = v.xmax, xerr = v.xerr;
  double band = 2.0 * xmax * xerr + xerr * xerr + 2.0 * v.dimp * 5.9604645e-8 * xmax * xmax;
  if (std::isfinite(base_min)) band += 1e-7 * (std::fabs(base_min) + 1.0);
  const float thr_lo = std::isfinite(base_min) ? f32_below(base_min - band) : -INFINITY;
  const float thr_hi = std::isfinite(base_min) ? -f32_below(-(base_min + band)) : -INFINITY;

  hipStream_t st = v.stream;
  // pair capacity: never below n (one row nominates at most n - 1 pairs, so a strip of one row always fits)
  int64_t cap = g_pair_cap;
  if (cap == 0) {
    size_t free_b = 0, total_b = 0;
    ANR_HIP(hipMemGetInfo(&free_b, &total_b));
    // room for 64 nominated pairs a row, within a quarter of the free memory; denser inputs go through the strips
    cap = std::min<int64_t>((int64_t)(free_b / 4) / kBytesPerPair, std::max<int64_t>(64 * n, 1 << 16));
    cap = std::min<int64_t>(cap, std::max<int64_t>(n * (n - 1) / 2, 1));
  }
  cap = std::min<int64_t>(std::max<int64_t>(cap, n), 1ll << 30);

  DevBuf<int> d_cluster, d_ids, d_nbr, d_cnt, d_inter, d_uni, r_col, r_inter, r_uni;
  DevBuf<int64_t> d_indptr;
  DevBuf<double> d_comb, d_base, r_comb, r_base;
  DevBuf<uint2> cand;
  DevBuf<unsigned long long> r_row, s_key, counters;
  DevBuf<unsigned> r_idx, s_val, seg;
  DevBuf<unsigned char> temp;
  const int64_t nm = n * M;
  ANR_TRY(d_cluster.alloc(n, "related"));
  ANR_TRY(d_indptr.alloc(n + 1, "related"));
  ANR_TRY(d_ids.alloc(nnz, "related"));
  ANR_TRY(d_nbr.alloc(nm, "related"));
  ANR_TRY(d_cnt.alloc(n, "related"));
  ANR_TRY(d_inter.alloc(nm, "related"));
  ANR_TRY(d_uni.alloc(nm, "related"));
  ANR_TRY(d_comb.alloc(nm, "related"));
  ANR_TRY(d_base.alloc(nm, "related"));
  ANR_TRY(seg.alloc(2 * n, "related"));
  ANR_TRY(counters.alloc(kRelCounters, "related"));
  ANR_TRY(cand.alloc(cap, "related", 0, "the nominated pairs"));
  ANR_TRY(r_row.alloc(2 * cap, "related", 0, "the kept pairs"));
  ANR_TRY(r_idx.alloc(2 * cap, "related", 0, "the kept pairs"));
  ANR_TRY(r_col.alloc(2 * cap, "related", 0, "the kept pairs"));
  ANR_TRY(r_inter.alloc(2 * cap, "related", 0, "the kept pairs"));
  ANR_TRY(r_uni.alloc(2 * cap, "related", 0, "the kept pairs"));
  ANR_TRY(r_comb.alloc(2 * cap, "related", 0, "the kept pairs"));
  ANR_TRY(r_base.alloc(2 * cap, "related", 0, "the kept pairs"));
  ANR_TRY(s_key.alloc(2 * cap, "related", 0, "the sorted records"));
  ANR_TRY(s_val.alloc(2 * cap, "related", 0, "the sorted records"));
  const size_t temp_bytes = radix_sort_temp_bytes(2 * cap);
  ANR_TRY(temp.alloc((int64_t)temp_bytes, "related", 0, "the sort"));
  const int64_t scratch = 4 * (d_cluster.cap + d_ids.cap + d_nbr.cap + d_cnt.cap + d_inter.cap + d_uni.cap + seg.cap) +
                          8 * (d_indptr.cap + d_comb.cap + d_base.cap + counters.cap + cand.cap) +
                          4 * (r_idx.cap + r_col.cap + r_inter.cap + r_uni.cap + s_val.cap) +
                          8 * (r_row.cap + r_comb.cap + r_base.cap + s_key.cap) + temp.cap;

  if (cluster) ANR_HIP(hipMemcpyAsync(d_cluster.p, cluster, (size_t)n * 4, hipMemcpyHostToDevice, st));
  else ANR_HIP(hipMemsetAsync(d_cluster.p, 0xff, (size_t)n * 4, st));
  ANR_HIP(hipMemcpyAsync(d_indptr.p, ent_indptr, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
  if (nnz > 0) ANR_HIP(hipMemcpyAsync(d_ids.p, ent_ids, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
  ANR_HIP(hipMemsetAsync(d_nbr.p, 0xff, (size_t)nm * 4, st));
  ANR_HIP(hipMemsetAsync(d_cnt.p, 0, (size_t)n * 4, st));
  ANR_HIP(hipMemsetAsync(d_inter.p, 0, (size_t)nm * 4, st));
  ANR_HIP(hipMemsetAsync(d_uni.p, 0, (size_t)nm * 4, st));
  ANR_HIP(hipMemsetAsync(d_comb.p, 0, (size_t)nm * 8, st));
  ANR_HIP(hipMemsetAsync(d_base.p, 0, (size_t)nm * 8, st));

  const int64_t n_tiles = ceil_div(n, kTileRows);
  const int nblk = (int)ceil_div(n_tiles, 8);
  constexpr int slots_bytes = 2 * 4 * 16 * 1024;
  ANR_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(&k_related_walk), slots_bytes));

  RelatedWalk wk{};
  wk.x16 = v.x16;
  wk.kb = v.kb;
  wk.n_rows = n;
  wk.n_tiles = n_tiles;
  wk.thr_lo = thr_lo;
  wk.thr_hi = thr_hi;
  wk.cluster = d_cluster.p;
  wk.exclude_same = excl;
  wk.cand = cand.p;
  wk.cap = (unsigned long long)cap;
  wk.counters = counters.p;

  RelatedScore sc{};
  sc.x32 = v.x32;
  sc.dim = v.dim;
  sc.cand = cand.p;
  sc.cluster = d_cluster.p;
  sc.indptr = d_indptr.p;
  sc.ids = d_ids.p;
  sc.threshold = thr;
  sc.thr_bonus = thr - 0.1;
  sc.one_minus_w = one_minus_w;
  sc.w = w;
  sc.bonus = bonus;
  sc.min_shared = p->min_shared;
  sc.exclude_same = excl;
  sc.rec_row = r_row.p;
  sc.rec_idx = r_idx.p;
  sc.rec_col = r_col.p;
  sc.rec_inter = r_inter.p;
  sc.rec_uni = r_uni.p;
  sc.rec_comb = r_comb.p;
  sc.rec_base = r_base.p;
  sc.counters = counters.p;

  RelatedSelect se{};
  se.n_rows = n;
  se.M = M;
  se.key = s_key.p;
  se.val = s_val.p;
  se.seg_lo = seg.p;
  se.seg_hi = seg.p + n;
  se.rec_col = r_col.p;
  se.rec_inter = r_inter.p;
  se.rec_uni = r_uni.p;
  se.rec_comb = r_comb.p;
  se.rec_base = r_base.p;
  se.nbr = d_nbr.p;
  se.n_nbr = d_cnt.p;
  se.inter = d_inter.p;
  se.uni = d_uni.p;
  se.comb = d_comb.p;
  se.base = d_base.p;

  Events<4> ev;
  if (g_timing) ANR_TRY(ev.init());
  float ms[3] = {0.f, 0.f, 0.f};
  int64_t nominated = 0, scored = 0, kept = 0, strips = 0, in_band = 0;
  unsigned long long hc[kRelCounters] = {};

  // strips of rows [lo, hi): a walk that nominates more than the capacity is walked again over fewer rows
  int64_t rows = n;
  for (int64_t lo = 0; lo < n;) {
    int64_t hi = std::min(n, lo + rows);
    ANR_TRY(ev.mark(0, st));
    for (;;) {
      const int bi0 = (int)(lo / 256), bi1 = (int)((hi - 1) / 256);
      wk.pg = make_patch_grid(bi1 - bi0 + 1, nblk);
      wk.n_slots = wk.pg.grid();
      wk.bi0 = bi0;
      wk.row_lo = (int)lo;
      wk.row_hi = (int)hi;
      ANR_HIP(hipMemsetAsync(counters.p, 0, kRelCounters * 8, st));
      const int64_t persistent = std::min<int64_t>(wk.n_slots, std::max(8, v.n_cu / 8 * 8));  // a multiple of 8: slot % 8 = XCD
      hipLaunchKernelGGL(k_related_walk, dim3((unsigned)persistent), dim3(512), slots_bytes, st, wk);
      ANR_HIP(hipGetLastError());
      ANR_HIP(hipMemcpyAsync(hc, counters.p, sizeof hc, hipMemcpyDeviceToHost, st));
      ANR_HIP(hipStreamSynchronize(st));
      nominated += (int64_t)hc[kRelCand];
      if (hc[kRelCand] <= (unsigned long long)cap) break;
      if (hi - lo == 1) return fail(ANR_EHIP, "related: one row nominated more pairs than there are rows");
      // the share of the strip that would have fitted, with a fifth to spare
      rows = std::max<int64_t>(1, (int64_t)((double)(hi - lo) * 0.8 * (double)cap / (double)hc[kRelCand]));
      hi = lo + rows;
    }
    ++strips;
    ANR_TRY(ev.mark(1, st));
    const unsigned long long n_cand = hc[kRelCand];
    in_band += (int64_t)hc[kRelBand];
    scored += (int64_t)n_cand;
    unsigned long long n_rec = 0;
    if (n_cand > 0) {
      sc.n_cand = n_cand;
      const unsigned grid = (unsigned)std::min<int64_t>(ceil_div((int64_t)n_cand, 256 / kSjPairLanes), (int64_t)v.n_cu * 32);
      hipLaunchKernelGGL(k_related_score, dim3(grid), dim3(256), 0, st, sc);
      ANR_HIP(hipGetLastError());
      ANR_HIP(hipMemcpyAsync(hc, counters.p, sizeof hc, hipMemcpyDeviceToHost, st));
      ANR_HIP(hipStreamSynchronize(st));
      n_rec = hc[kRelRecords];
    }
    ANR_TRY(ev.mark(2, st));
    if (n_rec > 0) {
      kept += (int64_t)(n_rec / 2);
      ANR_TRY(radix_sort_pairs_u64(temp.p, r_row.p, s_key.p, r_idx.p, s_val.p, (int64_t)n_rec, false, st));
      ANR_HIP(hipMemsetAsync(seg.p, 0, (size_t)n * 8, st));
      se.n_rec = n_rec;
      hipLaunchKernelGGL(k_related_segments, dim3((unsigned)ceil_div((int64_t)n_rec, 256)), dim3(256), 0, st, se);
      ANR_HIP(hipGetLastError());
      hipLaunchKernelGGL(k_related_select, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, st, se);
      ANR_HIP(hipGetLastError());
    }
    ANR_TRY(ev.mark(3, st));
    if (ev.on) {
      ANR_HIP(hipStreamSynchronize(st));
      for (int k = 0; k < 3; ++k) {
        float t = 0.f;
        ANR_TRY(ev.elapsed(k, k + 1, &t));
        ms[k] += t;
      }
    }
    lo = hi;
    // a strip that used less than a quarter of the capacity: try twice the rows next
    if (n_cand < (unsigned long long)cap / 4) rows = std::min<int64_t>(n, rows * 2);
  }

  ANR_HIP(hipMemcpyAsync(nbr_host, d_nbr.p, (size_t)nm * 4, hipMemcpyDeviceToHost, st));
  ANR_HIP(hipMemcpyAsync(n_nbr_host, d_cnt.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  if (comb_host) ANR_HIP(hipMemcpyAsync(comb_host, d_comb.p, (size_t)nm * 8, hipMemcpyDeviceToHost, st));
  if (base_host) ANR_HIP(hipMemcpyAsync(base_host, d_base.p, (size_t)nm * 8, hipMemcpyDeviceToHost, st));
  if (inter_host) ANR_HIP(hipMemcpyAsync(inter_host, d_inter.p, (size_t)nm * 4, hipMemcpyDeviceToHost, st));
  if (uni_host) ANR_HIP(hipMemcpyAsync(uni_host, d_uni.p, (size_t)nm * 4, hipMemcpyDeviceToHost, st));
  ANR_HIP(hipStreamSynchronize(st));
  if (ev.on) std::copy(ms, ms + 3, g_times);
  if (stats) {
    stats[0] = nominated;
    stats[1] = scored;
    stats[2] = kept;
    stats[3] = strips;
    stats[4] = cap;
    stats[5] = in_band;
    stats[6] = scratch;
    stats[7] = 0;
  }
  return ANR_OK;
}
