// anr_index_diversify (include/anorag.h): semantic dedup and greedy diverse selection of fused candidates — the arithmetic
// of the reference's DiversityScheduler.schedule_candidates (retrieval/diversity_scheduler.py:523) for a batch of queries.
// k_div_gram + k_div_cosine build one C x C float64 cosine matrix per query from the index's stored rows (f64 MFMA);
// k_div_select runs the decision procedure on it, one workgroup per query.  gram_f64.hpp has the lane map and the
// determinism rule, DESIGN.md §5g the tile layout and the error bound.  Compiled without multiply-add contraction
// (Makefile, EXACT).
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

constexpr int kDivMaxC = 1024;  // candidates per query
constexpr int kDivTile = 32;    // a workgroup's tile of one query's matrix: 2 x 2 waves of 16 x 16
constexpr int kDivLd = kGramKC + 1;
constexpr int kDivNT = 256;

struct DivGram {
  const float *x32;
  int dim;
  const int64_t *rows;  // [total] row ids
  const int64_t *offs;  // [nq + 1]
  const int64_t *soff;  // [nq] first element of query q's matrix
  const int *tiles;     // [n_tiles][3]: query, tile row, tile column (row <= column)
  double *G;
  double *nrm;          // [total] sqrt(G_ii)
};

// Raw products G = A A^T of one 32 x 32 tile: the shared tile (gram_f64.hpp) with 2 x 2 waves of one 16 x 16 block each.
// Result register r of a lane is row 16 wi + (lane >> 4) + 4 r, column 16 wj + (lane & 15).
__global__ __launch_bounds__(kDivNT) void k_div_gram(DivGram p) {
  __shared__ float As[kDivTile][kDivLd], Bs[kDivTile][kDivLd];
  __shared__ int64_t ra[kDivTile], rb[kDivTile];
  const int q = p.tiles[3 * blockIdx.x], bi = p.tiles[3 * blockIdx.x + 1], bj = p.tiles[3 * blockIdx.x + 2];
  const int64_t o = p.offs[q];
  const int C = (int)(p.offs[q + 1] - o);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wi = w >> 1, wj = w & 1;
  if (tid < kDivTile) {
    const int ia = bi * kDivTile + tid, ib = bj * kDivTile + tid;
    ra[tid] = ia < C ? p.rows[o + ia] : -1;
    rb[tid] = ib < C ? p.rows[o + ib] : -1;
  }
  __syncthreads();
  double4_t acc[1];
  gram_f64_tile<2, 2, 1, kDivLd>(p.x32, p.dim, ra, rb, As, Bs, acc);
  double *G = p.G + p.soff[q];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = bi * kDivTile + wi * 16 + (lane >> 4) + 4 * r, j = bj * kDivTile + wj * 16 + (lane & 15);
    if (i < C && j < C) {
      const double v = acc[0][r];
      G[(int64_t)i * C + j] = v;
      if (bi != bj) G[(int64_t)j * C + i] = v;  // tiles below the diagonal are not computed
      if (i == j) p.nrm[o + i] = sqrt(v);
    }
  }
}

struct DivCosine {
  const int64_t *offs, *soff;
  const int *rowq;  // [total] query of a candidate
  const double *nrm;
  double *G;
};

// sim = clamp(G_ij / (|a_i| |a_j|), 0, 1), 0 where a norm is zero; one workgroup per matrix row, in place
__global__ __launch_bounds__(kDivNT) void k_div_cosine(DivCosine p) {
  const int q = p.rowq[blockIdx.x];
  const int64_t o = p.offs[q];
  const int C = (int)(p.offs[q + 1] - o), i = (int)(blockIdx.x - o);
  double *row = p.G + p.soff[q] + (int64_t)i * C;
  const double ni = p.nrm[o + i];
  for (int j = threadIdx.x; j < C; j += kDivNT) {
    const double nj = p.nrm[o + j];
    double s = 0.0;
    if (ni != 0.0 && nj != 0.0) {
      s = row[j] / (ni * nj);
      s = s < 1.0 ? s : 1.0;   // Python's min(1.0, s)
      s = s > 0.0 ? s : 0.0;   // max(0.0, .)
    }
    row[j] = s;
  }
}

struct DivSelect {
  const double *sim;
  const int64_t *offs, *soff, *koff;
  const double *score;
  const unsigned *types;  // may be nullptr
  anr_diversity_params prm;
  int *kept, *n_kept, *sel, *n_sel;
  double *sel_sim;
};

// quota balance bonus (:761-779) of a type mask under the current counts, types in ascending bit order
__device__ __forceinline__ double div_bonus(unsigned m, const int *cnt, const anr_diversity_params &prm) {
  double bonus = 0.0;
  for (int t = 0; t < 32; ++t) {
    if (!((m >> t) & 1u)) continue;
    const int quota = prm.quotas[t];
    if (quota > 0) {
      const double fill = (double)cnt[t] / (double)quota;
      if (fill < prm.balance_factor) bonus += (prm.balance_factor - fill) * 0.5;
    }
  }
  return bonus;
}

// The decision procedure of one query: dedup, pass-through or stable sort, quota round one, greedy fill.  Threads own
// candidates (strided); every branch below is taken by the whole workgroup on values read from LDS after a barrier.
__global__ __launch_bounds__(kDivNT) void k_div_select(DivSelect a) {
  __shared__ int kept[kDivMaxC], srt[kDivMaxC], sel[kDivMaxC];
  __shared__ double sc[kDivMaxC], S[kDivMaxC];
  __shared__ unsigned char taken[kDivMaxC];
  __shared__ int cnt[32];
  __shared__ int s_hit, s_nk, s_nsel, s_pick;
  __shared__ double rv[kDivNT / 64];
  __shared__ int rp[kDivNT / 64];
  const int q = blockIdx.x, tid = threadIdx.x;
  const int64_t o = a.offs[q];
  const int C = (int)(a.offs[q + 1] - o);
  const int maxc = a.prm.max_candidates;
  if (C == 0) {
    if (tid == 0) {
      a.n_kept[q] = 0;
      a.n_sel[q] = 0;
    }
    return;
  }
  const double *sim = a.sim + a.soff[q];
  for (int c = tid; c < C; c += kDivNT) sc[c] = a.score[o + c];
  if (tid == 0) s_nk = 0;
  __syncthreads();

  // 1. dedup (:383-401)
  if (!a.prm.dedup) {
    for (int c = tid; c < C; c += kDivNT) kept[c] = c;
    if (tid == 0) s_nk = C;
    __syncthreads();
  } else {
    const double thr = a.prm.similarity_threshold;
    for (int i = 0; i < C; ++i) {
      const int nk = s_nk;
      if (tid == 0) s_hit = INT_MAX;
      __syncthreads();
      const double *row = sim + (int64_t)i * C;
      for (int p = tid; p < nk; p += kDivNT)
        if (row[kept[p]] >= thr) atomicMin(&s_hit, p);  // the first kept entry that is similar enough
      __syncthreads();
      const int hit = s_hit;
      if (hit == INT_MAX) {
        if (tid == 0) {
          kept[nk] = i;
          s_nk = nk + 1;
        }
      } else if (sc[i] > sc[kept[hit]]) {
        // remove the entry, close the gap, append the new candidate
        int tmp[kDivMaxC / kDivNT];
#pragma unroll
        for (int m = 0; m < kDivMaxC / kDivNT; ++m) {
          const int p = hit + tid + m * kDivNT;
          tmp[m] = p < nk - 1 ? kept[p + 1] : 0;
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < kDivMaxC / kDivNT; ++m) {
          const int p = hit + tid + m * kDivNT;
          if (p < nk - 1) kept[p] = tmp[m];
        }
        if (tid == 0) kept[nk - 1] = i;
      }
      __syncthreads();
    }
  }
  const int nk = s_nk;
  for (int p = tid; p < nk; p += kDivNT) a.kept[o + p] = kept[p];
  if (tid == 0) a.n_kept[q] = nk;

  int nsel;
  if (nk <= maxc) {
    // 2. pass-through (:655): the kept list, unsorted
    for (int p = tid; p < nk; p += kDivNT) sel[p] = kept[p];
    nsel = nk;
    __syncthreads();
  } else {
    // 3. stable sort by score descending: rank = entries with a greater score, or an equal one and an earlier position
    for (int p = tid; p < nk; p += kDivNT) {
      const double sp = sc[kept[p]];
      int rank = 0;
      for (int r = 0; r < nk; ++r) {
        const double sr = sc[kept[r]];
        rank += (sr > sp || (sr == sp && r < p)) ? 1 : 0;
      }
      srt[rank] = kept[p];
      taken[p] = 0;
    }
    if (tid < 32) cnt[tid] = 0;
    __syncthreads();
    // 4. quota round one (:698-719), or the plain form's first pick (:666)
    if (tid == 0) {
      int n = 0;
      if (a.prm.quota) {
        for (int pos = 0; pos < nk && n < maxc; ++pos) {
          const unsigned m = a.types ? a.types[o + srt[pos]] : 0u;
          bool avail = false;
          for (int t = 0; t < 32; ++t)
            if (((m >> t) & 1u) && cnt[t] < a.prm.quotas[t]) avail = true;
          if (avail) {
            sel[n++] = srt[pos];
            taken[pos] = 1;
            for (int t = 0; t < 32; ++t)
              if ((m >> t) & 1u) ++cnt[t];
          }
        }
      } else {
        sel[0] = srt[0];
        taken[0] = 1;
        n = 1;
      }
      s_nsel = n;
    }
    __syncthreads();
    // 5. greedy fill (:669-685, :724-754); S = sum of sim to the selected, in selection order
    {
      const int n0 = s_nsel;
      for (int pos = tid; pos < nk; pos += kDivNT) {
        double s = 0.0;
        if (!taken[pos])
          for (int e = 0; e < n0; ++e) s += sim[(int64_t)sel[e] * C + srt[pos]];
        S[pos] = s;
      }
    }
    for (;;) {
      const int n = s_nsel;
      if (n >= maxc || n >= nk) break;
      double best = -1.0;
      int bpos = INT_MAX;
      for (int pos = tid; pos < nk; pos += kDivNT) {
        if (taken[pos]) continue;
        const int c = srt[pos];
        const double score = sc[c];
        double gain = 1.0;  // nothing selected yet (:784)
        if (n > 0) {
          const double avg = S[pos] / (double)n;
          const double div = 1.0 - avg;
          const double ns = score < 1.0 ? score : 1.0;
          gain = 0.7 * div + 0.3 * ns;
        }
        double v = gain;
        if (a.prm.quota) {
          const double bonus = div_bonus(a.types ? a.types[o + c] : 0u, cnt, a.prm);
          v = score * 0.5 + gain * 0.3 + bonus * 0.2;
        }
        if (v > best) {  // ascending positions: a tie keeps the earlier one
          best = v;
          bpos = pos;
        }
      }
      for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_down(best, off);
        const int op = __shfl_down(bpos, off);
        if (ov > best || (ov == best && op < bpos)) {
          best = ov;
          bpos = op;
        }
      }
      if ((tid & 63) == 0) {
        rv[tid >> 6] = best;
        rp[tid >> 6] = bpos;
      }
      __syncthreads();
      if (tid == 0) {
        for (int w = 1; w < kDivNT / 64; ++w)
          if (rv[w] > best || (rv[w] == best && rp[w] < bpos)) {
            best = rv[w];
            bpos = rp[w];
          }
        if (bpos == INT_MAX) {
          s_pick = -1;  // nothing above -1.0: the selection stops short
        } else {
          sel[n] = srt[bpos];
          taken[bpos] = 1;
          s_nsel = n + 1;
          s_pick = bpos;
          const unsigned m = a.types ? a.types[o + srt[bpos]] : 0u;
          for (int t = 0; t < 32; ++t)
            if ((m >> t) & 1u) ++cnt[t];
        }
      }
      __syncthreads();
      const int pick = s_pick;
      if (pick < 0) break;
      const double *row = sim + (int64_t)srt[pick] * C;
      for (int pos = tid; pos < nk; pos += kDivNT)
        if (!taken[pos]) S[pos] += row[srt[pos]];
      __syncthreads();
    }
    nsel = s_nsel;
  }
  // 6. outputs
  for (int e = tid; e < nsel; e += kDivNT) a.sel[o + e] = sel[e];
  if (tid == 0) a.n_sel[q] = nsel;
  double *ks = a.sel_sim + a.koff[q];
  for (int e = tid; e < nsel * nsel; e += kDivNT) ks[e] = sim[(int64_t)sel[e / nsel] * C + sel[e % nsel]];
}

// developer timing (anr_diversify_timing): HIP-event times of the last timed call
bool g_timing = false;
float g_times[3] = {0.f, 0.f, 0.f};  // similarity kernels, decision kernel, first copy in to last copy out

// byte offsets of the arrays of one call inside the arena, every one 8-byte aligned
struct Layout {
  size_t offs, soff, koff, rows, score, types, rowq, tiles, in_end;  // inputs: one copy to the device
  size_t nrm;
  size_t kept, sel, n_kept, n_sel, sel_sim, out_end;                 // outputs: one copy back
};

int run(DevBuf<unsigned char> &sim_buf, DevBuf<unsigned char> &arena, const float *x32, int dim, int64_t ntotal, int64_t nq,
        const int64_t *offs, const int64_t *rows, const double *sim_host, const double *scores, const uint32_t *types,
        const anr_diversity_params &prm, int32_t *kept, int32_t *n_kept, int32_t *selected, int32_t *n_selected,
        double *sel_sim, hipStream_t st) {
  const int64_t total = offs[nq];
  std::vector<int64_t> soff((size_t)nq), koff((size_t)nq);
  std::vector<int> tiles;
  int64_t stotal = 0, ktotal = 0;
  for (int64_t q = 0; q < nq; ++q) {
    const int64_t C = offs[q + 1] - offs[q];
    soff[q] = stotal;
    koff[q] = ktotal;
    stotal += C * C;
    const int64_t K = std::min<int64_t>(C, prm.max_candidates);
    ktotal += K * K;
    if (!sim_host) {
      const int nb = (int)ceil_div(C, kDivTile);
      for (int bi = 0; bi < nb; ++bi)
        for (int bj = bi; bj < nb; ++bj) {
          tiles.push_back((int)q);
          tiles.push_back(bi);
          tiles.push_back(bj);
        }
    }
  }
  const int64_t n_tiles = (int64_t)tiles.size() / 3;
  if (nq > 0x7fffffffLL || total > 0x7fffffffLL || n_tiles > 0x7fffffffLL)
    return fail(ANR_EINVAL, "diversify: too many queries or candidates for one call");

  Layout L{};
  ArenaLayout<8> lay;
  L.offs = lay.take((size_t)(nq + 1) * 8);
  L.soff = lay.take((size_t)nq * 8);
  L.koff = lay.take((size_t)nq * 8);
  L.rows = lay.take(sim_host ? 0 : (size_t)total * 8);
  L.score = lay.take((size_t)total * 8);
  L.types = lay.take(types ? (size_t)total * 4 : 0);
  L.rowq = lay.take(sim_host ? 0 : (size_t)total * 4);
  L.tiles = lay.take(tiles.size() * 4);
  L.in_end = lay.at;
  L.nrm = lay.take((size_t)total * 8);
  L.kept = lay.take((size_t)total * 4);
  L.sel = lay.take((size_t)total * 4);
  L.n_kept = lay.take((size_t)nq * 4);
  L.n_sel = lay.take((size_t)nq * 4);
  L.sel_sim = lay.take((size_t)ktotal * 8);
  L.out_end = lay.at;

  // both grow by a quarter beyond the need
  ANR_TRY(arena.alloc((int64_t)L.out_end, "diversify", (int64_t)(L.out_end + L.out_end / 4), "the candidate arrays"));
  ANR_TRY(sim_buf.alloc(stotal * 8, "diversify", stotal * 10, "the similarity matrices"));
  unsigned char *A = arena.p;
  double *sim = reinterpret_cast<double *>(sim_buf.p);

  std::vector<unsigned char> in(L.in_end, 0);
  memcpy(&in[L.offs], offs, (size_t)(nq + 1) * 8);
  memcpy(&in[L.soff], soff.data(), (size_t)nq * 8);
  memcpy(&in[L.koff], koff.data(), (size_t)nq * 8);
  memcpy(&in[L.score], scores, (size_t)total * 8);
  if (types) memcpy(&in[L.types], types, (size_t)total * 4);
  if (!sim_host) {
    memcpy(&in[L.rows], rows, (size_t)total * 8);
    int *rowq = reinterpret_cast<int *>(&in[L.rowq]);
    for (int64_t q = 0; q < nq; ++q)
      for (int64_t c = offs[q]; c < offs[q + 1]; ++c) rowq[c] = (int)q;
    if (!tiles.empty()) memcpy(&in[L.tiles], tiles.data(), tiles.size() * 4);
  }
  Events<5> ev;
  if (g_timing) ANR_TRY(ev.init());
  ANR_TRY(ev.mark(0, st));
  ANR_HIP(hipMemcpyAsync(A, in.data(), L.in_end, hipMemcpyHostToDevice, st));

  ANR_TRY(ev.mark(1, st));
  if (sim_host) {
    ANR_HIP(hipMemcpyAsync(sim, sim_host, (size_t)stotal * 8, hipMemcpyHostToDevice, st));
  } else {
    DivGram g{x32,
              dim,
              reinterpret_cast<const int64_t *>(A + L.rows),
              reinterpret_cast<const int64_t *>(A + L.offs),
              reinterpret_cast<const int64_t *>(A + L.soff),
              reinterpret_cast<const int *>(A + L.tiles),
              sim,
              reinterpret_cast<double *>(A + L.nrm)};
    hipLaunchKernelGGL(k_div_gram, dim3((unsigned)n_tiles), dim3(kDivNT), 0, st, g);
    ANR_HIP(hipGetLastError());
    DivCosine c{g.offs, g.soff, reinterpret_cast<const int *>(A + L.rowq), g.nrm, g.G};
    hipLaunchKernelGGL(k_div_cosine, dim3((unsigned)total), dim3(kDivNT), 0, st, c);
    ANR_HIP(hipGetLastError());
  }

  ANR_TRY(ev.mark(2, st));
  DivSelect s{};
  s.sim = sim;
  s.offs = reinterpret_cast<const int64_t *>(A + L.offs);
  s.soff = reinterpret_cast<const int64_t *>(A + L.soff);
  s.koff = reinterpret_cast<const int64_t *>(A + L.koff);
  s.score = reinterpret_cast<const double *>(A + L.score);
  s.types = types ? reinterpret_cast<const unsigned *>(A + L.types) : nullptr;
  s.prm = prm;
  s.kept = reinterpret_cast<int *>(A + L.kept);
  s.sel = reinterpret_cast<int *>(A + L.sel);
  s.n_kept = reinterpret_cast<int *>(A + L.n_kept);
  s.n_sel = reinterpret_cast<int *>(A + L.n_sel);
  s.sel_sim = reinterpret_cast<double *>(A + L.sel_sim);
  hipLaunchKernelGGL(k_div_select, dim3((unsigned)nq), dim3(kDivNT), 0, st, s);
  ANR_HIP(hipGetLastError());
  ANR_TRY(ev.mark(3, st));

  std::vector<unsigned char> out(L.out_end - L.kept);
  ANR_HIP(hipMemcpyAsync(out.data(), A + L.kept, out.size(), hipMemcpyDeviceToHost, st));
  ANR_TRY(ev.mark(4, st));
  ANR_HIP(hipStreamSynchronize(st));
  if (ev.on) {
    ANR_TRY(ev.elapsed(1, 2, &g_times[0]));
    ANR_TRY(ev.elapsed(2, 3, &g_times[1]));
    ANR_TRY(ev.elapsed(0, 4, &g_times[2]));
  }
  const unsigned char *O = out.data() - L.kept;
  for (int64_t q = 0; q < nq; ++q) {
    const int64_t o = offs[q];
    const int nk = reinterpret_cast<const int *>(O + L.n_kept)[q], ns = reinterpret_cast<const int *>(O + L.n_sel)[q];
    if (kept) memcpy(kept + o, O + L.kept + (size_t)o * 4, (size_t)nk * 4);
    if (selected) memcpy(selected + o, O + L.sel + (size_t)o * 4, (size_t)ns * 4);
    if (n_kept) n_kept[q] = nk;
    if (n_selected) n_selected[q] = ns;
    if (sel_sim) memcpy(sel_sim + koff[q], O + L.sel_sim + (size_t)koff[q] * 8, (size_t)ns * ns * 8);
  }
  return ANR_OK;
}

}  // namespace

extern "C" int anr_diversify_timing(int32_t enable, float *ms3) {
  g_timing = enable != 0;
  if (ms3) std::copy(g_times, g_times + 3, ms3);
  return ANR_OK;
}

extern "C" int anr_index_diversify(anr_index *h, int32_t device, int64_t nq, const int64_t *offs, const int64_t *rows_host,
                                   const double *sim_host, const double *scores_host, const uint32_t *type_masks_host,
                                   const anr_diversity_params *p, int32_t *kept, int32_t *n_kept, int32_t *selected,
                                   int32_t *n_selected, double *sel_sim) {
  if (!h && !sim_host) return fail(ANR_EINVAL, "diversify: null handle without a similarity matrix");
  if (nq < 0) return fail(ANR_EINVAL, "diversify: nq must be >= 0");
  if (nq == 0) return ANR_OK;
  if (!offs || !p) return fail(ANR_EINVAL, "diversify: null offs or parameters");
  if (p->max_candidates < 1) return fail(ANR_EINVAL, "diversify: max_candidates must be >= 1");
  if (!(p->similarity_threshold == p->similarity_threshold) || !(p->balance_factor == p->balance_factor))
    return fail(ANR_EINVAL, "diversify: the threshold and the balance factor must be numbers");
  if (offs[0] != 0) return fail(ANR_EINVAL, "diversify: offs must start at 0");
  for (int64_t q = 0; q < nq; ++q) {
    const int64_t C = offs[q + 1] - offs[q];
    if (C < 0) return fail(ANR_EINVAL, "diversify: offs must ascend");
    if (C > kDivMaxC) return fail(ANR_EINVAL, "diversify: query %lld has %lld candidates (limit %d)", (long long)q, (long long)C, kDivMaxC);
  }
  const int64_t total = offs[nq];
  if (total == 0) {
    if (n_kept) std::fill(n_kept, n_kept + nq, 0);
    if (n_selected) std::fill(n_selected, n_selected + nq, 0);
    return ANR_OK;
  }
  if (!scores_host) return fail(ANR_EINVAL, "diversify: null scores");
  if (!sim_host && !rows_host) return fail(ANR_EINVAL, "diversify: null rows");

  if (!h) {
    DeviceGuard g(device);
    if (!g.ok) return fail(ANR_EHIP, "hipSetDevice(%d) failed", device);
    DevBuf<unsigned char> sim, arena;  // of this call only
    return run(sim, arena, nullptr, 0, 0, nq, offs, nullptr, sim_host, scores_host, type_masks_host, *p, kept, n_kept, selected,
               n_selected, sel_sim, nullptr);
  }
  const IndexCore c = index_core(h);
  DeviceGuard g(c.device);
  if (!g.ok) return fail(ANR_EHIP, "hipSetDevice(%d) failed", c.device);
  std::lock_guard<std::mutex> lk(*c.mu);
  const IndexCore cur = index_core(h);  // under the lock: an add may have moved the rows
  if (!sim_host)
    for (int64_t e = 0; e < total; ++e)
      if (rows_host[e] < 0 || rows_host[e] >= cur.ntotal)
        return fail(ANR_EINVAL, "diversify: row id %lld outside [0, %lld)", (long long)rows_host[e], (long long)cur.ntotal);
  IndexScratch &sc = index_scratch(h);
  return run(sc.div_sim, sc.div_arena, cur.x32, cur.dim, cur.ntotal, nq, offs, rows_host, sim_host, scores_host,
             type_masks_host, *p, kept, n_kept, selected, n_selected, sel_sim, cur.stream);
}
