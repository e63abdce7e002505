// IVF-Flat index (anr_ivf_*, include/anorag.h): device k-means, list-ordered storage, probed scan with exact re-score.
//
// Storage.  Every row ever added stays in `xall` (float32, preprocessed, indexed by its global id) beside its list
// (`assign`) and an alive flag.  The searched copy is list-ordered: rows of list 0, then list 1, ..., each list padded to
// whole 32-row tiles, as float32 (`xs`, the exact re-score and nothing else), as f16 (`x16`, what the probed scan reads),
// with the global id of each row (`ids`, -1 on padding) and its squared norm in f64 (`n2`).  Inside a list rows are in
// ascending id order; the list-ordered copy is rebuilt from `xall` before the first search / list_sizes after any add /
// remove / centroid change, so it depends on (centroids, alive rows) only: adding in chunks or at once gives the same
// bytes.  Memory: the rows live twice in float32 (`xall`, `xs`) and once in f16; removed rows stay in `xall`.
//
// Assignment (training, add).  k_assign scores 64 rows x 64 centroids per step in float32 (LDS-staged FMA tiles) and keeps
// each row's best and second key (IP: x.c; L2: 2 x.c - |c|^2, the row's own |x|^2 drops out).  Where the two are closer
// than the float32 error bound of the keys, k_assign_fix re-scores the row against every centroid in float64 (IP: x.c;
// L2: -|x - c|^2).  The result is the float64 argmax, ties to the lower list id.
//
// Training: Lloyd's iterations.  Per iteration: assign, count, stable-sort the row numbers by list (radix_sort.hip), one
// mean per list summed in float64 in ascending row order (k_seg_mean; no atomics, so two trainings are bit-identical).
// An empty list j (ascending j) takes the second half of the currently largest list b (lowest id among equals; only if
// b holds at least 2 rows): b keeps its first ceil(n_b / 2) rows in ascending row order, j the rest, and both become the
// means of their halves.  With the spherical option (the facade sets it for inner product, as faiss's IVF does) every
// centroid is normalised after the update.
//
// Search.  Coarse: every query against every centroid in float64 (k_coarse), the nprobe best lists (ties to the lower
// id; k_topp).  The (query, list) pairs of the batch are grouped by list on the host, so each probed 32-row tile is read
// once for all queries that probe its list (k_probe: f16 rows x float32 query, float32 accumulation).  k_select keeps the
// K' best approximate keys of each query (radix select), re-scores them from the float32 rows in float64, orders them by
// (score, id) and checks the certificate: the k-th exact key must exceed the K'-th approximate key plus the f16 / float32
// error bound; the rows left out then cannot reach the top-k.  A query whose certificate fails is re-scored exactly over
// all its probed rows (k_exhaust).  Results are the exact top-k of the probed lists' float32 rows.
//
// IVF-PQ (anr_ivf_create_pq).  The same handle with a product quantiser: everything above up to the list order is shared
// (coarse k-means, assignment, probing, the radix select).  A row is stored as its list and m code bytes; code j is the
// nearest of 256 codebook entries (dsub = dim / m values) to sub-vector j of the residual x - c_list, found by the
// assignment above run on all m sub-spaces in one launch (k_pq_assign, strided sub-vectors, L2, float64 re-check of near
// ties in k_pq_assign_fix).  The preprocessed float32 rows, lists and codes are kept on the host in insertion order;
// the device keeps the centroids, the codebooks and the list-ordered codes with their ids: each list padded to 64-row
// tiles, a tile stored as [m4 = ceil(m / 4)][64 rows][4 code bytes], so a wave loads one code dword per lane, 256
// contiguous bytes.  The PQ k-means (k_pq_keys, k_pq_seg_mean) sorts the (sub-space, code) of every training row with
// the same radix sort and takes the same float64 segment means and empty-entry split as the coarse k-means.  Search
// (ADC): the coarse pass as above, then k_pq_scan per (query, list, up to 8 tiles): the m x 256 float32 LUT in LDS (IP:
// the query's LUT from k_pq_lut, q_j . cb_j[c]; L2: built per list, |(q - c_l)_j - cb_j[c]|^2), one ds_read_b32 lookup
// per code byte, float32 accumulation in ascending j; k_pq_select keeps the k best keys (radix select, no re-score)
// ordered by (key, id).  Results are the ADC top-k of the probed lists, which is faiss's IndexIVFPQ answer.
#include <algorithm>
#include <cmath>
#include <cfloat>
#include <mutex>
#include <numeric>
#include <vector>

#include <hip/hip_fp16.h>

#include "common.hpp"

namespace anr {

constexpr int kIvfMaxDim = 2048;    // the probed scan stages 32 f16 rows per workgroup in LDS
constexpr int kIvfMaxNlist = 8192;  // the coarse top-nprobe sorts one query's nlist keys in LDS
constexpr int kIvfMaxK = 1024;
constexpr int kSelCap = 2048;       // candidates kept by k_select (K' plus ties at the threshold)
constexpr int kTile = 32;

// ---------------------------------------------------------------------------------------------------------------
// device helpers

__device__ __forceinline__ unsigned f2ord(float v) {
  unsigned u = __float_as_uint(v);
  if ((u << 1) == 0u) u = 0u;
  return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(unsigned o) { return __uint_as_float((o >> 31) ? (o & 0x7fffffffu) : ~o); }

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// (key, id) before (key', id'): larger key first, then smaller id
template <typename I>
__device__ __forceinline__ bool better(double ka, I ia, double kb, I ib) {
  return ka > kb || (ka == kb && ia < ib);
}

// in-LDS bitonic sort of n2 (a power of two) (key, id) pairs, best first
template <typename I>
__device__ void bitonic_sort(double *key, I *id, int n2) {
  for (int size = 2; size <= n2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = threadIdx.x; i < (n2 >> 1); i += blockDim.x) {
        const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
        const bool first_block = (lo & size) == 0;
        const bool hi_better = better(key[hi], id[hi], key[lo], id[lo]);
        if (hi_better == first_block) {
          const double tk = key[lo];
          key[lo] = key[hi];
          key[hi] = tk;
          const I ti = id[lo];
          id[lo] = id[hi];
          id[hi] = ti;
        }
      }
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// kernels

// preprocess n rows (normalise when asked, exactly as the flat index does: divide by the f32 of the f64 norm) into out;
// nrm[i] = || out row ||
__global__ __launch_bounds__(256) void k_ivf_prep(const float *in, int64_t n, int dim, int normalize, float *out, float *nrm) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  const float *x = in + r * dim;
  float *y = out + r * dim;
  double acc = 0.0;
  for (int k = lane; k < dim; k += 64) {
    const double v = (double)x[k];
    acc += v * v;
  }
  acc = wave_sum(acc);
  const float s = (float)sqrt(acc);
  const bool div = normalize && s != 0.0f;
  double acc2 = 0.0;
  for (int k = lane; k < dim; k += 64) {
    const float v = div ? x[k] / s : x[k];
    y[k] = v;
    acc2 += (double)v * (double)v;
  }
  acc2 = wave_sum(acc2);
  if (lane == 0) nrm[r] = (float)sqrt(acc2);
}

// centroid statistics: cn2[c] = f32(|c|^2), cnrm[c] = f32(|c|)
__global__ __launch_bounds__(256) void k_ivf_cstat(const float *cent, int nlist, int dim, float *cn2, float *cnrm) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= nlist) return;
  double acc = 0.0;
  for (int k = lane; k < dim; k += 64) {
    const double v = (double)cent[(int64_t)c * dim + k];
    acc += v * v;
  }
  acc = wave_sum(acc);
  if (lane == 0) {
    cn2[c] = (float)acc;
    cnrm[c] = (float)sqrt(acc);
  }
}

// the float32 tile pass of the assignment: 64 rows of x (row stride ldx, dim values each) against nlist centroids (rows
// of dim values, back to back); the best centroid of row r goes to out[r * ostride], and a row whose best two keys are
// within the error bound goes to fix[] as r * fmul + fadd.  rnrm[r * rstride] = |row r|, cmax >= every |centroid|.
__device__ __forceinline__ void assign_tiles(const float *x, int64_t ldx, int64_t n, int dim, const float *cent,
                                             const float *cn2, int nlist, int l2, const float *rnrm, int64_t rstride,
                                             float cmax, int32_t *out, int64_t ostride, int32_t *fix, int fmul, int fadd,
                                             int32_t *nfix, float (*As)[68], float (*Bs)[68]) {
  const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
  const int64_t row0 = (int64_t)blockIdx.x * 64;
  float b1[4], b2[4];
  int i1[4];
  for (int i = 0; i < 4; ++i) {
    b1[i] = -INFINITY;
    b2[i] = -INFINITY;
    i1[i] = 0x7fffffff;
  }
  for (int c0 = 0; c0 < nlist; c0 += 64) {
    float acc[4][4] = {};
    for (int k0 = 0; k0 < dim; k0 += 16) {
      for (int e = tid; e < 1024; e += 256) {
        const int r = e >> 4, kk = e & 15, gk = k0 + kk;
        const int64_t gr = row0 + r;
        const int gc = c0 + r;
        As[kk][r] = (gr < n && gk < dim) ? x[gr * ldx + gk] : 0.0f;
        Bs[kk][r] = (gc < nlist && gk < dim) ? cent[(int64_t)gc * dim + gk] : 0.0f;
      }
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) {
        float a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          a[i] = As[kk][tr * 4 + i];
          b[i] = Bs[kk][tc * 4 + i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
      }
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + tc * 4 + j;
      if (c >= nlist) continue;
      const float cc = l2 ? cn2[c] : 0.0f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float key = l2 ? 2.0f * acc[i][j] - cc : acc[i][j];
        if (key > b1[i]) {  // c ascends within a thread: an equal key keeps the lower id
          b2[i] = b1[i];
          b1[i] = key;
          i1[i] = c;
        } else if (key > b2[i]) {
          b2[i] = key;
        }
      }
    }
  }
  // merge the 16 column threads of each row group (lanes tc = 0..15 are consecutive lanes of one wave)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    for (int off = 8; off > 0; off >>= 1) {
      const float o1 = __shfl_xor(b1[i], off), o2 = __shfl_xor(b2[i], off);
      const int oi = __shfl_xor(i1[i], off);
      if (o1 > b1[i] || (o1 == b1[i] && oi < i1[i])) {
        b2[i] = fmaxf(b1[i], o2);
        b1[i] = o1;
        i1[i] = oi;
      } else {
        b2[i] = fmaxf(b2[i], o1);
      }
    }
  }
  if (tc != 0) return;
  const float u = 5.9604645e-8f;  // 2^-24
  const float g = (float)(dim + 4) * u * 1.01f;
  for (int i = 0; i < 4; ++i) {
    const int64_t r = row0 + tr * 4 + i;
    if (r >= n) continue;
    out[r * ostride] = i1[i];
    if (nlist < 2) continue;
    const float xn = rnrm[r * rstride];
    float bound = l2 ? 2.0f * (2.0f * g * xn * cmax + cmax * cmax * u + (2.0f * xn * cmax + cmax * cmax) * u)
                     : 2.0f * (g * xn * cmax + xn * cmax * u);
    bound = bound * 1.5f + 1e-30f;
    if (!(b1[i] - b2[i] > bound)) {
      const int s = atomicAdd(nfix, 1);
      fix[s] = (int32_t)r * fmul + fadd;
    }
  }
}

// top-1 list of n rows (see the file comment); rows whose best two keys are within the error bound go to fix[]
__global__ __launch_bounds__(256) void k_ivf_assign(const float *x, int64_t n, int dim, const float *cent, const float *cn2,
                                                    int nlist, int l2, const float *rnrm, float cmax, int32_t *out,
                                                    int32_t *fix, int32_t *nfix) {
  __shared__ float As[16][68];
  __shared__ float Bs[16][68];
  assign_tiles(x, dim, n, dim, cent, cn2, nlist, l2, rnrm, 1, cmax, out, 1, fix, 1, 0, nfix, As, Bs);
}

// float64 argmax of one row xrow (dim values) over nlist centroids (IP: x.c, L2: -|x - c|^2; ties to the lower id) to
// *dst; one 256-thread workgroup
__device__ __forceinline__ void assign_fix_row(const float *xrow, int dim, const float *cent, int nlist, int l2,
                                               double *xr, double *wk, int *wi, int32_t *dst) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = threadIdx.x; k < dim; k += 256) xr[k] = (double)xrow[k];
  __syncthreads();
  double bk = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = wave; c < nlist; c += 4) {
    const float *cr = cent + (int64_t)c * dim;
    double acc = 0.0;
    for (int k = lane; k < dim; k += 64) {
      const double cv = (double)cr[k];
      if (l2) {
        const double d = xr[k] - cv;
        acc += d * d;
      } else {
        acc += xr[k] * cv;
      }
    }
    acc = wave_sum(acc);
    const double key = l2 ? -acc : acc;
    if (key > bk) {
      bk = key;
      bi = c;
    }
  }
  if (lane == 0) {
    wk[wave] = bk;
    wi[wave] = bi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double k0 = wk[0];
    int i0 = wi[0];
    for (int w = 1; w < 4; ++w)
      if (better(wk[w], wi[w], k0, i0)) {
        k0 = wk[w];
        i0 = wi[w];
      }
    *dst = i0;
  }
}

// float64 argmax over all centroids for the rows listed in fix[] (IP: x.c, L2: -|x - c|^2; ties to the lower id)
__global__ __launch_bounds__(256) void k_ivf_assign_fix(const float *x, int dim, const float *cent, int nlist, int l2,
                                                        const int32_t *fix, const int32_t *nfix, int32_t *out) {
  __shared__ double xr[kIvfMaxDim];
  __shared__ double wk[4];
  __shared__ int wi[4];
  if ((int)blockIdx.x >= *nfix) return;
  const int64_t r = fix[blockIdx.x];
  assign_fix_row(x + r * dim, dim, cent, nlist, l2, xr, wk, wi, out + r);
}

// sort keys for the list order: alive rows by list, the rest after the last list
__global__ void k_ivf_keys(const int32_t *assign, const uint8_t *alive, int64_t n, int nlist, unsigned long long *keys,
                           unsigned *vals, int32_t *counts) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool a = alive == nullptr || alive[i];
  const int l = a ? assign[i] : nlist;
  keys[i] = (unsigned long long)l;
  vals[i] = (unsigned)i;
  if (a) atomicAdd(&counts[l], 1);
}

// one mean per list over its segment of the sorted row numbers, summed in float64 in segment order
__global__ __launch_bounds__(256) void k_ivf_seg_mean(const float *x, int dim, const unsigned *rows, const int64_t *seg,
                                                      float *cent) {
  const int l = blockIdx.x;
  const int64_t s0 = seg[2 * l], cnt = seg[2 * l + 1];
  if (cnt <= 0) return;
  for (int d = threadIdx.x; d < dim; d += 256) {
    double s = 0.0;
    for (int64_t i = 0; i < cnt; ++i) s += (double)x[(int64_t)rows[s0 + i] * dim + d];
    cent[(int64_t)l * dim + d] = (float)(s / (double)cnt);
  }
}

// list-ordered copy: sorted position p -> padded row list_off[l] + (p - seg_start[l])
__global__ __launch_bounds__(256) void k_ivf_gather(const float *xall, int dim, const unsigned long long *keys,
                                                    const unsigned *vals, int64_t nalive, const int64_t *list_off,
                                                    const int64_t *seg_start, float *xs, __half *x16, int64_t *ids,
                                                    double *n2) {
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= nalive) return;
  const int l = (int)keys[p];
  const int64_t id = vals[p];
  const int64_t dst = list_off[l] + (p - seg_start[l]);
  const float *src = xall + id * dim;
  double acc = 0.0;
  for (int k = lane; k < dim; k += 64) {
    const float v = src[k];
    xs[dst * dim + k] = v;
    x16[dst * dim + k] = __float2half_rn(v);
    acc += (double)v * (double)v;
  }
  acc = wave_sum(acc);
  if (lane == 0) {
    ids[dst] = id;
    n2[dst] = acc;
  }
}

// rows of the given global ids, back to back
__global__ __launch_bounds__(256) void k_ivf_rows(const float *xall, int dim, const int64_t *ids, int64_t n, float *out) {
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const float *src = xall + ids[i] * dim;
  for (int k = threadIdx.x & 63; k < dim; k += 64) out[i * dim + k] = src[k];
}

// coarse scores in float64: cs[q, c] (IP: q.c; L2: -|q - c|^2); grid (nq, ceil(nlist / 64))
__global__ __launch_bounds__(256) void k_ivf_coarse(const float *q, int dim, const float *cent, int nlist, int l2,
                                                    double *cs) {
  __shared__ double qr[kIvfMaxDim];
  const int64_t qi = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = threadIdx.x; k < dim; k += 256) qr[k] = (double)q[qi * dim + k];
  __syncthreads();
  const int c0 = blockIdx.y * 64 + wave * 16;
  for (int c = c0; c < c0 + 16 && c < nlist; ++c) {
    const float *cr = cent + (int64_t)c * dim;
    double acc = 0.0;
    for (int k = lane; k < dim; k += 64) {
      const double cv = (double)cr[k];
      if (l2) {
        const double d = qr[k] - cv;
        acc += d * d;
      } else {
        acc += qr[k] * cv;
      }
    }
    acc = wave_sum(acc);
    if (lane == 0) cs[qi * nlist + c] = l2 ? -acc : acc;
  }
}

// the nprobe best lists of each query (ties to the lower id); dynamic LDS: n2 * (8 + 4) bytes
__global__ __launch_bounds__(1024) void k_ivf_topp(const double *cs, int nlist, int n2, int nprobe, int32_t *probe) {
  extern __shared__ double sh[];
  double *key = sh;
  int *id = reinterpret_cast<int *>(sh + n2);
  const int64_t qi = blockIdx.x;
  for (int i = threadIdx.x; i < n2; i += blockDim.x) {
    key[i] = i < nlist ? cs[qi * nlist + i] : -INFINITY;
    id[i] = i < nlist ? i : 0x7fffffff;
  }
  __syncthreads();
  bitonic_sort(key, id, n2);
  for (int j = threadIdx.x; j < nprobe; j += blockDim.x) probe[qi * nprobe + j] = id[j];
}

struct ProbeItem {
  int64_t row0;    // first padded row of the tile
  int64_t tile0;   // tile's row offset inside its list
  int32_t e0, e1;  // its list's (query, segment offset) entries
};

// approximate keys of every probed row: f16 rows x float32 query, float32 accumulation.  IP: q.x; L2: 2 q.x - |x|^2 -
// |q|^2 (= -|q - x|^2); padding rows -inf.  out[cbase[q] + seg + tile0 + r] = key, pos[...] = padded row
__global__ __launch_bounds__(256) void k_ivf_probe(const __half *x16, const int64_t *ids, const double *n2, int dim,
                                                   const float *q, const float *qn2, int l2, const ProbeItem *items,
                                                   const int32_t *eq, const int64_t *eoff, const int64_t *cbase,
                                                   float *key_out, int32_t *pos_out) {
  extern __shared__ __half2 tile[];  // 32 rows of dim / 2 half2, row stride dim / 2 + 1
  const ProbeItem it = items[blockIdx.x];
  const int dh = dim >> 1, stride = dh + 1;
  const __half2 *src = reinterpret_cast<const __half2 *>(x16 + it.row0 * dim);
  for (int i = threadIdx.x; i < kTile * dh; i += 256) {
    const int r = i / dh, p = i - r * dh;
    tile[r * stride + p] = src[i];
  }
  __syncthreads();
  const int r = threadIdx.x >> 3, s = threadIdx.x & 7;
  const int64_t row = it.row0 + r;
  const bool pad = ids[row] < 0;
  const float xn2 = (float)n2[row];
  const __half2 *tr = tile + r * stride;
  for (int e = it.e0; e < it.e1; ++e) {
    const int qi = eq[e];
    const float2 *qv = reinterpret_cast<const float2 *>(q + (int64_t)qi * dim);
    float acc = 0.0f;
    for (int p = s; p < dh; p += 8) {
      const float2 h = __half22float2(tr[p]);
      const float2 v = qv[p];
      acc = fmaf(h.x, v.x, acc);
      acc = fmaf(h.y, v.y, acc);
    }
    acc += __shfl_xor(acc, 1);
    acc += __shfl_xor(acc, 2);
    acc += __shfl_xor(acc, 4);
    if (s == 0) {
      const int64_t o = cbase[qi] + eoff[e] + it.tile0 + r;
      key_out[o] = pad ? -INFINITY : (l2 ? 2.0f * acc - xn2 - qn2[qi] : acc);
      pos_out[o] = (int32_t)row;
    }
  }
}

// exact key of padded row `row` for query qv: IP q.x, L2 -|q - x|^2 (float64 accumulation); one wave
__device__ __forceinline__ double exact_key(const float *xs, int64_t row, const float *qv, int dim, int l2, int lane) {
  const float *x = xs + row * dim;
  double acc = 0.0;
  for (int k = lane; k < dim; k += 64) {
    const double a = (double)qv[k], b = (double)x[k];
    if (l2) {
      const double d = a - b;
      acc += d * d;
    } else {
      acc += a * b;
    }
  }
  acc = wave_sum(acc);
  return l2 ? -acc : acc;
}

__device__ __forceinline__ void write_topk(const double *key, const int64_t *id, int m, int k, int l2, float *D, int64_t *I) {
  for (int j = threadIdx.x; j < k; j += blockDim.x) {
    if (j < m && id[j] >= 0 && id[j] != INT64_MAX) {
      D[j] = l2 ? (float)(-key[j]) : (float)key[j];
      I[j] = id[j];
    } else {
      D[j] = l2 ? FLT_MAX : -FLT_MAX;
      I[j] = -1;
    }
  }
}

// radix select over the S float keys kq (-inf = padding): T = the ordered form (f2ord) of the kp-th largest key and
// remaining = how many of the kp best are equal to it; all = true when at most kp keys are not padding (T and
// remaining are then unused).  Every thread of the block calls it; hist: 256 words of LDS, s_*: LDS scalars.
__device__ __forceinline__ void radix_threshold(const float *kq, int64_t S, int kp, unsigned *hist, unsigned *s_prefix,
                                                unsigned *s_remaining, unsigned *s_valid, unsigned &prefix,
                                                unsigned &remaining, bool &all) {
  const int tid = threadIdx.x;
  const unsigned ninf = f2ord(-INFINITY);
  // pass 0 also counts the rows that are not padding
  unsigned mask = 0;
  prefix = 0;
  remaining = (unsigned)kp;
  all = false;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (tid < 256) hist[tid] = 0;
    if (tid == 0) *s_valid = 0;
    __syncthreads();
    unsigned nv = 0;
    for (int64_t i = tid; i < S; i += blockDim.x) {
      const unsigned o = f2ord(kq[i]);
      if (o != ninf) ++nv;
      if ((o & mask) == prefix) atomicAdd(&hist[(o >> shift) & 255u], 1u);
    }
    if (pass == 0) atomicAdd(s_valid, nv);
    __syncthreads();
    if (pass == 0 && *s_valid <= (unsigned)kp) {
      all = true;
      break;
    }
    if (tid == 0) {
      unsigned cum = 0;
      int b = 255;
      for (; b > 0; --b) {
        if (cum + hist[b] >= remaining) break;
        cum += hist[b];
      }
      *s_remaining = remaining - cum;
      *s_prefix = prefix | ((unsigned)b << shift);
    }
    __syncthreads();
    prefix = *s_prefix;
    remaining = *s_remaining;
    mask |= 255u << shift;
    __syncthreads();
  }
}

// per query: K' best approximate keys (radix select), float64 re-score, (score, id) order, certificate
__global__ __launch_bounds__(1024) void k_ivf_select(const float *keys, const int32_t *pos, const int64_t *cbase,
                                                     const int64_t *ctot, const float *xs, const int64_t *ids,
                                                     const float *q, int dim, int l2, int k, int kp,
                                                     const float *qbound, float *D, int64_t *I, int32_t *fail) {
  __shared__ unsigned hist[256];
  __shared__ unsigned s_prefix, s_remaining, s_cnt_gt, s_cnt_eq, s_valid;
  __shared__ double ck[kSelCap];
  __shared__ int64_t cid[kSelCap];
  __shared__ int32_t cpos[kSelCap];
  const int64_t qi = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const float *kq = keys + cbase[qi];
  const int32_t *pq = pos + cbase[qi];
  const int64_t S = ctot[qi];
  const unsigned ninf = f2ord(-INFINITY);

  unsigned prefix = 0, remaining = 0;
  bool all = false;
  radix_threshold(kq, S, kp, hist, &s_prefix, &s_remaining, &s_valid, prefix, remaining, all);
  // collect: keys above the threshold, then keys equal to it up to the capacity (all others are <= threshold)
  if (tid == 0) {
    s_cnt_gt = 0;
    s_cnt_eq = 0;
  }
  __syncthreads();
  const unsigned T = prefix;
  const unsigned ngt = all ? 0u : (unsigned)kp - remaining;
  for (int64_t i = tid; i < S; i += blockDim.x) {
    const unsigned o = f2ord(kq[i]);
    if (all) {
      if (o != ninf) {
        const unsigned sl = atomicAdd(&s_cnt_gt, 1u);
        cpos[sl] = pq[i];
      }
    } else if (o > T) {
      const unsigned sl = atomicAdd(&s_cnt_gt, 1u);
      cpos[sl] = pq[i];
    } else if (o == T) {
      const unsigned sl = ngt + atomicAdd(&s_cnt_eq, 1u);
      if (sl < (unsigned)kSelCap) cpos[sl] = pq[i];
    }
  }
  __syncthreads();
  const int m = all ? (int)s_cnt_gt : (int)min((unsigned)kSelCap, ngt + s_cnt_eq);
  int n2 = 1;
  while (n2 < m) n2 <<= 1;
  if (n2 < 2) n2 = 2;
  const float *qv = q + qi * dim;
  for (int c = wave; c < n2; c += nw) {
    if (c < m) {
      const double e = exact_key(xs, cpos[c], qv, dim, l2, lane);
      if (lane == 0) {
        ck[c] = e;
        cid[c] = ids[cpos[c]];
      }
    } else if (lane == 0) {
      ck[c] = -INFINITY;
      cid[c] = INT64_MAX;
    }
  }
  __syncthreads();
  bitonic_sort(ck, cid, n2);
  write_topk(ck, cid, m, k, l2, D + qi * k, I + qi * k);
  if (tid == 0) {
    bool ok = true;
    if (!all) ok = ck[k - 1] > (double)ord2f(T) + (double)qbound[qi];
    fail[qi] = ok ? 0 : 1;
  }
}

// exact top-k over every probed row of the listed queries: running top-k merged with chunks of float64 keys
__global__ __launch_bounds__(1024) void k_ivf_exhaust(const int32_t *qlist, const float *keys, const int32_t *pos,
                                                      const int64_t *cbase, const int64_t *ctot, const float *xs,
                                                      const int64_t *ids, const float *q, int dim, int l2, int k,
                                                      float *D, int64_t *I) {
  __shared__ double ck[kSelCap];
  __shared__ int64_t cid[kSelCap];
  const int64_t qi = qlist[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const int32_t *pq = pos + cbase[qi];
  const int64_t S = ctot[qi];
  const float *qv = q + qi * dim;
  for (int i = tid; i < kSelCap; i += blockDim.x) {
    ck[i] = -INFINITY;
    cid[i] = INT64_MAX;
  }
  __syncthreads();
  const int chunk = kSelCap - k;
  for (int64_t s0 = 0; s0 < S; s0 += chunk) {
    for (int c = wave; c < chunk; c += nw) {
      const int64_t i = s0 + c;
      double e = -INFINITY;
      int64_t id = INT64_MAX;
      if (i < S && ids[pq[i]] >= 0) {  // padding by id: an f16 key may be -inf or NaN on a real row
        e = exact_key(xs, pq[i], qv, dim, l2, lane);
        id = ids[pq[i]];
      }
      if (lane == 0) {
        ck[k + c] = e;
        cid[k + c] = id;
      }
    }
    __syncthreads();
    bitonic_sort(ck, cid, kSelCap);
  }
  write_topk(ck, cid, kSelCap, k, l2, D + qi * k, I + qi * k);
}

// ---------------------------------------------------------------------------------------------------------------
// product quantiser (anr_ivf_create_pq; see "IVF-PQ" at the top of the file)

constexpr int kPqMaxM = 128;      // one float32 LUT of m x 256 entries in LDS
constexpr int kPqTile = 64;       // list rows per code tile: one row per lane of a wave
constexpr int kPqItemTiles = 8;   // tiles per scan workgroup
constexpr int kPqNiter = 25;      // faiss's ClusteringParameters default (the PQ's own k-means)
constexpr int64_t kPqChunk = 1 << 18;  // rows per encoding step

// r = x - c_assign(x) in float32, one wave per row
__global__ __launch_bounds__(256) void k_pq_residual(const float *x, int64_t n, int dim, const float *cent,
                                                     const int32_t *asg, float *res) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  const float *c = cent + (int64_t)asg[r] * dim;
  for (int k = threadIdx.x & 63; k < dim; k += 64) res[r * dim + k] = x[r * dim + k] - c[k];
}

// nearest codebook entry of every sub-vector: grid (ceil(n / 64), m), sub-space j = blockIdx.y.  The residual rows are
// [n][m][dsub]; codes go to out[r * m + j] and near ties to fix[] as r * m + j (k_pq_assign_fix)
__global__ __launch_bounds__(256) void k_pq_assign(const float *res, int64_t n, int dim, int dsub, int m, const float *cb,
                                                   const float *cbn2, const float *rnrm, const float *cbmax, int32_t *out,
                                                   int32_t *fix, int32_t *nfix) {
  __shared__ float As[16][68];
  __shared__ float Bs[16][68];
  const int j = blockIdx.y;
  assign_tiles(res + (int64_t)j * dsub, dim, n, dsub, cb + (int64_t)j * 256 * dsub, cbn2 + j * 256, 256, 1, rnrm + j, m,
               cbmax[j], out + j, m, fix, m, j, nfix, As, Bs);
}

// float64 argmin of |r_j - cb_j[c]|^2 (ties to the lower code) for the sub-vectors listed in fix[]
__global__ __launch_bounds__(256) void k_pq_assign_fix(const float *res, int dsub, int m, const float *cb,
                                                       const int32_t *fix, const int32_t *nfix, int32_t *out) {
  __shared__ double xr[kIvfMaxDim];
  __shared__ double wk[4];
  __shared__ int wi[4];
  if ((int)blockIdx.x >= *nfix) return;
  const int64_t e = fix[blockIdx.x];
  const int j = (int)(e % m);
  assign_fix_row(res + e * dsub, dsub, cb + (int64_t)j * 256 * dsub, 256, 1, xr, wk, wi, out + e);
}

// sort keys of the PQ k-means: entry e = j * n + r -> key j * 256 + code of (r, j), value r; counts per (j, code)
__global__ void k_pq_keys(const int32_t *codes, int64_t n, int m, unsigned long long *keys, unsigned *vals,
                          int32_t *counts) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * m) return;
  const int j = (int)(e / n);
  const int64_t r = e - (int64_t)j * n;
  const int key = j * 256 + codes[r * m + j];
  keys[e] = (unsigned long long)key;
  vals[e] = (unsigned)r;
  atomicAdd(&counts[key], 1);
}

// one codebook entry l = j * 256 + c per block: the float64 mean, in segment order, of sub-vector j of its rows
__global__ __launch_bounds__(64) void k_pq_seg_mean(const float *res, int dim, int dsub, const unsigned *rows,
                                                    const int64_t *seg, float *cb) {
  const int l = blockIdx.x, j = l >> 8;
  const int64_t s0 = seg[2 * l], cnt = seg[2 * l + 1];
  if (cnt <= 0) return;
  for (int d = threadIdx.x; d < dsub; d += 64) {
    double s = 0.0;
    for (int64_t i = 0; i < cnt; ++i) s += (double)res[(int64_t)rows[s0 + i] * dim + j * dsub + d];
    cb[(int64_t)l * dsub + d] = (float)(s / (double)cnt);
  }
}

__global__ void k_pq_pack(const int32_t *in, int64_t n, uint8_t *out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (uint8_t)in[i];
}

// list-ordered codes: sorted position p -> padded row dst = list_off[l] + (p - seg_start[l]); byte j of row dst sits at
// ((dst / 64 * m4 + j / 4) * 64 + dst % 64) * 4 + j % 4, so one wave reads one code dword per lane, 256 contiguous bytes
__global__ void k_pq_gather(const uint8_t *codes, int m, int m4, const unsigned long long *keys, const unsigned *vals,
                            int64_t nalive, const int64_t *list_off, const int64_t *seg_start, uint8_t *lcodes,
                            int64_t *ids) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nalive) return;
  const int l = (int)keys[p];
  const int64_t id = vals[p];
  const int64_t dst = list_off[l] + (p - seg_start[l]);
  const int64_t t = dst / kPqTile, lane = dst % kPqTile;
  for (int j = 0; j < m; ++j) lcodes[((t * m4 + (j >> 2)) * kPqTile + lane) * 4 + (j & 3)] = codes[id * m + j];
  ids[dst] = id;
}

// inner-product LUT of each query: lut[(q * mp + j) * 256 + c] = q_j . cb_j[c] (float32, ascending d), 0 for j >= m;
// grid (nq, mp)
__global__ __launch_bounds__(256) void k_pq_lut(const float *q, int dim, int dsub, int m, const float *cb, float *lut) {
  const int64_t qi = blockIdx.x;
  const int j = blockIdx.y, c = threadIdx.x;
  float acc = 0.0f;
  if (j < m) {
    const float *qv = q + qi * dim + j * dsub;
    const float *cv = cb + ((int64_t)j * 256 + c) * dsub;
    for (int d = 0; d < dsub; ++d) acc = fmaf(qv[d], cv[d], acc);
  }
  lut[(qi * gridDim.y + j) * 256 + c] = acc;
}

struct PqItem {
  int64_t tile;   // first code tile
  int64_t out;    // first candidate slot of the query's segment
  int32_t qi, l;  // query, list
  int32_t ntiles;
};

// ADC keys of up to kPqItemTiles tiles of one probed list for one query.  The LUT (mp x 256 float32, zero rows past m)
// sits in LDS: IP copies the query's LUT, L2 builds |(q - c_l)_j - cb_j[c]|^2 for this list.  One row per lane, one
// ds_read_b32 lookup per code byte, float32 accumulation in ascending j.  IP key: q.c_l (the float64 coarse score) +
// sum; L2 key: -sum; padding rows -inf.  out[it.out + t * 64 + lane] = key, pos[...] = padded row
template <int L2>
__global__ __launch_bounds__(256) void k_pq_scan(const PqItem *items, const uint32_t *codes, const int64_t *ids, int m4,
                                                 int dsub, int dim, const float *lut, const float *q, const float *cent,
                                                 const float *cb, int m, const double *cs, int nl, float *key_out,
                                                 int32_t *pos_out) {
  extern __shared__ float sl[];  // 4 m4 x 256 LUT entries, then (L2) q - c_l
  const PqItem it = items[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nlut = m4 * 1024;
  if (L2) {
    float *a = sl + nlut;
    const float *qv = q + (int64_t)it.qi * dim, *cv = cent + (int64_t)it.l * dim;
    for (int k = tid; k < dim; k += 256) a[k] = qv[k] - cv[k];
    __syncthreads();
    for (int e = tid; e < nlut; e += 256) {  // e = j * 256 + c
      const int j = e >> 8;
      float acc = 0.0f;
      if (j < m) {
        const float *bv = cb + (int64_t)e * dsub, *av = a + j * dsub;
        for (int d = 0; d < dsub; ++d) {
          const float t = av[d] - bv[d];
          acc = fmaf(t, t, acc);
        }
      }
      sl[e] = acc;
    }
  } else {
    const float4 *src = reinterpret_cast<const float4 *>(lut + (int64_t)it.qi * nlut);
    float4 *dst = reinterpret_cast<float4 *>(sl);
    for (int e = tid; e < (nlut >> 2); e += 256) dst[e] = src[e];
  }
  __syncthreads();
  const double base = L2 ? 0.0 : cs[(int64_t)it.qi * nl + it.l];
  for (int t = wave; t < it.ntiles; t += 4) {
    const int64_t tile = it.tile + t;
    const uint32_t *src = codes + tile * m4 * kPqTile + lane;
    float acc = 0.0f;
#pragma unroll 4
    for (int w = 0; w < m4; ++w) {
      const uint32_t v = src[w * kPqTile];
      const float *lw = sl + w * 1024;
      acc += lw[v & 255u];
      acc += lw[256 + ((v >> 8) & 255u)];
      acc += lw[512 + ((v >> 16) & 255u)];
      acc += lw[768 + (v >> 24)];
    }
    const int64_t row = tile * kPqTile + lane;
    const float key = L2 ? -acc : (float)(base + (double)acc);
    const int64_t o = it.out + (int64_t)t * kPqTile + lane;
    key_out[o] = ids[row] < 0 ? -INFINITY : key;
    pos_out[o] = (int32_t)row;
  }
}

// per query: the k best ADC keys (radix select), ordered by (key desc, id asc); rows tied with the k-th key are kept
// up to kSelCap candidates in all
__global__ __launch_bounds__(1024) void k_pq_select(const float *keys, const int32_t *pos, const int64_t *cbase,
                                                    const int64_t *ctot, const int64_t *ids, int l2, int k, float *D,
                                                    int64_t *I) {
  __shared__ unsigned hist[256];
  __shared__ unsigned s_prefix, s_remaining, s_cnt_gt, s_cnt_eq, s_valid;
  __shared__ double ck[kSelCap];
  __shared__ int64_t cid[kSelCap];
  const int64_t qi = blockIdx.x;
  const int tid = threadIdx.x;
  const float *kq = keys + cbase[qi];
  const int32_t *pq = pos + cbase[qi];
  const int64_t S = ctot[qi];
  const unsigned ninf = f2ord(-INFINITY);
  unsigned T = 0, remaining = 0;
  bool all = false;
  radix_threshold(kq, S, k, hist, &s_prefix, &s_remaining, &s_valid, T, remaining, all);
  if (tid == 0) {
    s_cnt_gt = 0;
    s_cnt_eq = 0;
  }
  __syncthreads();
  const unsigned ngt = all ? 0u : (unsigned)k - remaining;
  for (int64_t i = tid; i < S; i += blockDim.x) {
    const unsigned o = f2ord(kq[i]);
    unsigned sl = (unsigned)kSelCap;
    if (all ? o != ninf : o > T) sl = atomicAdd(&s_cnt_gt, 1u);
    else if (!all && o == T) sl = ngt + atomicAdd(&s_cnt_eq, 1u);
    if (sl < (unsigned)kSelCap) {
      ck[sl] = (double)kq[i];
      cid[sl] = ids[pq[i]];
    }
  }
  __syncthreads();
  const int m = all ? (int)s_cnt_gt : (int)min((unsigned)kSelCap, ngt + s_cnt_eq);
  int n2 = 1;
  while (n2 < m) n2 <<= 1;
  if (n2 < 2) n2 = 2;
  for (int c = m + tid; c < n2; c += blockDim.x) {
    ck[c] = -INFINITY;
    cid[c] = INT64_MAX;
  }
  __syncthreads();
  bitonic_sort(ck, cid, n2);
  write_topk(ck, cid, m, k, l2, D + qi * k, I + qi * k);
}

// ---------------------------------------------------------------------------------------------------------------
// host side

// room for n elements in a buffer that grows by half beyond what it holds, so that adds in chunks do not reallocate
// every time
template <typename T>
static int need(DevBuf<T> &b, int64_t n) {
  return b.alloc(n, "ivf", b.cap + b.cap / 2);
}

static uint64_t splitmix(uint64_t &s) {
  uint64_t z = (s += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

}  // namespace anr

using namespace anr;

struct anr_ivf {
  int dim = 0, metric = 0, normalize = 0, nlist = 0, device = 0, add_raw = 0, spherical = 0;
  bool dirty = false;             // the list-ordered copy lags behind the rows / centroids
  int64_t last_nq = 0, last_exhaust = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;
  bool trained = false;
  DevBuf<float> cent, cn2, cnrm;
  float cmax = 0.0f;
  // every row ever added, by global id
  DevBuf<float> xall, xnrm;
  DevBuf<int32_t> assign;
  DevBuf<uint8_t> alive_d;
  std::vector<uint8_t> alive;
  int64_t n_all = 0, n_alive = 0;
  float max_norm = 0.0f;
  // list-ordered copy
  DevBuf<float> xs;
  DevBuf<__half> x16;
  DevBuf<int64_t> ids;
  DevBuf<double> n2;
  std::vector<int64_t> list_cnt, list_off;  // alive rows per list; first padded row per list (nlist + 1 entries)
  // scratch
  DevBuf<unsigned long long> skeys, skeys2;
  DevBuf<unsigned> svals, svals2;
  DevBuf<char> stemp;
  DevBuf<int32_t> counts, fix, nfix;
  DevBuf<int64_t> seg, off_d;
  DevBuf<float> qbuf, qnrm, qn2, qbound, ckey, Dd;
  DevBuf<double> cs;
  DevBuf<int32_t> probe, cpos, failq, qlist;
  DevBuf<int64_t> cbase, ctot, eoff, Id, rid;
  DevBuf<float> rout;
  DevBuf<int32_t> eq;
  DevBuf<ProbeItem> items;
  std::vector<float> host_tmp;
  // product quantiser (pq): the rows, their lists and codes live on the host in insertion order; the device keeps the
  // codebooks and the list-ordered codes (lcodes) with their ids
  bool pq = false, pq_ready = false;  // PQ mode; codebooks present
  int m = 0, m4 = 0, dsub = 0;         // sub-spaces, code dwords per row, values per sub-space
  DevBuf<float> cb, cbn2, cbnrm, cbmax;   // [m][256][dsub]; |entry|^2, |entry|; per sub-space max |entry| (the bound)
  std::vector<float> xh;
  std::vector<int32_t> assign_h;
  std::vector<uint8_t> codes_h;        // [n_all][m]
  DevBuf<uint32_t> lcodes;
  DevBuf<float> lut;
  DevBuf<PqItem> pitems;
};

namespace {

int reencode_all(anr_ivf *h);
int rebuild_pq(anr_ivf *h);
int add_pq(anr_ivf *h, const float *x, int64_t n, bool host);
int search_pq(anr_ivf *h, const float *qin, bool host, int64_t nq, int k, int nprobe, float *D, int64_t *I);

int stage_rows(anr_ivf *h, const float *x, int64_t n, bool host, float *out, float *nrm, bool raw = false) {
  // raw rows to `out` (device), then preprocessed in place
  if (n == 0) return ANR_OK;
  if (host) ANR_HIP(hipMemcpyAsync(out, x, (size_t)n * h->dim * 4, hipMemcpyHostToDevice, h->stream));
  else if (x != out) ANR_HIP(hipMemcpyAsync(out, x, (size_t)n * h->dim * 4, hipMemcpyDeviceToDevice, h->stream));
  hipLaunchKernelGGL(k_ivf_prep, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, h->stream, out, n, h->dim,
                     h->normalize && !raw ? 1 : 0, out, nrm);
  ANR_HIP(hipGetLastError());
  return ANR_OK;
}

int update_cstats(anr_ivf *h) {
  hipLaunchKernelGGL(k_ivf_cstat, dim3((unsigned)ceil_div(h->nlist, 4)), dim3(256), 0, h->stream, h->cent.p, h->nlist,
                     h->dim, h->cn2.p, h->cnrm.p);
  ANR_HIP(hipGetLastError());
  std::vector<float> cn(h->nlist);
  ANR_HIP(hipMemcpyAsync(cn.data(), h->cnrm.p, (size_t)h->nlist * 4, hipMemcpyDeviceToHost, h->stream));
  ANR_HIP(hipStreamSynchronize(h->stream));
  h->cmax = 0.0f;
  for (float v : cn) h->cmax = std::max(h->cmax, v);
  h->cmax *= 1.0001f;
  return ANR_OK;
}

// list of each of n preprocessed rows x (norms xn) -> out
int assign_rows(anr_ivf *h, const float *x, const float *xn, int64_t n, int32_t *out) {
  if (n == 0) return ANR_OK;
  ANR_TRY(need(h->fix, n));
  ANR_TRY(need(h->nfix, 1));
  ANR_HIP(hipMemsetAsync(h->nfix.p, 0, 4, h->stream));
  const int l2 = h->metric == ANR_METRIC_L2;
  hipLaunchKernelGGL(k_ivf_assign, dim3((unsigned)ceil_div(n, 64)), dim3(256), 0, h->stream, x, n, h->dim, h->cent.p,
                     h->cn2.p, h->nlist, l2, xn, h->cmax, out, h->fix.p, h->nfix.p);
  ANR_HIP(hipGetLastError());
  int32_t nf = 0;
  ANR_HIP(hipMemcpyAsync(&nf, h->nfix.p, 4, hipMemcpyDeviceToHost, h->stream));
  ANR_HIP(hipStreamSynchronize(h->stream));
  if (nf > 0) {
    hipLaunchKernelGGL(k_ivf_assign_fix, dim3((unsigned)nf), dim3(256), 0, h->stream, x, h->dim, h->cent.p, h->nlist, l2,
                       h->fix.p, h->nfix.p, out);
    ANR_HIP(hipGetLastError());
  }
  return ANR_OK;
}

// stable sort of rows [0, n) by list (dead rows last); counts per list to `cnt`
int sort_by_list(anr_ivf *h, const int32_t *assign, const uint8_t *alive, int64_t n, std::vector<int64_t> &cnt) {
  ANR_TRY(need(h->skeys, n));
  ANR_TRY(need(h->skeys2, n));
  ANR_TRY(need(h->svals, n));
  ANR_TRY(need(h->svals2, n));
  ANR_TRY(need(h->stemp, (int64_t)radix_sort_temp_bytes(n)));
  ANR_TRY(need(h->counts, h->nlist + 1));
  ANR_HIP(hipMemsetAsync(h->counts.p, 0, (size_t)(h->nlist + 1) * 4, h->stream));
  hipLaunchKernelGGL(k_ivf_keys, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, h->stream, assign, alive, n, h->nlist,
                     h->skeys.p, h->svals.p, h->counts.p);
  ANR_HIP(hipGetLastError());
  ANR_TRY(radix_sort_pairs_u64(h->stemp.p, h->skeys.p, h->skeys2.p, h->svals.p, h->svals2.p, n, false, h->stream));
  std::vector<int32_t> c(h->nlist);
  ANR_HIP(hipMemcpyAsync(c.data(), h->counts.p, (size_t)h->nlist * 4, hipMemcpyDeviceToHost, h->stream));
  ANR_HIP(hipStreamSynchronize(h->stream));
  cnt.assign(c.begin(), c.end());
  return ANR_OK;
}

// rebuild the list-ordered copy from xall / assign / alive
int rebuild(anr_ivf *h) {
  const int nl = h->nlist;
  h->list_cnt.assign(nl, 0);
  h->list_off.assign(nl + 1, 0);
  if (h->n_all > 0) ANR_TRY(sort_by_list(h, h->assign.p, h->alive_d.p, h->n_all, h->list_cnt));
  std::vector<int64_t> seg_start(nl);
  int64_t s = 0;
  for (int l = 0; l < nl; ++l) {
    seg_start[l] = s;
    s += h->list_cnt[l];
    h->list_off[l + 1] = h->list_off[l] + round_up(h->list_cnt[l], kTile);
  }
  const int64_t npad = std::max<int64_t>(h->list_off[nl], kTile);
  const int dim = h->dim;
  ANR_TRY(need(h->xs, npad * dim));
  ANR_TRY(need(h->x16, npad * dim));
  ANR_TRY(need(h->ids, npad));
  ANR_TRY(need(h->n2, npad));
  ANR_TRY(need(h->off_d, 2 * nl));
  ANR_HIP(hipMemsetAsync(h->xs.p, 0, (size_t)npad * dim * 4, h->stream));
  ANR_HIP(hipMemsetAsync(h->x16.p, 0, (size_t)npad * dim * 2, h->stream));
  ANR_HIP(hipMemsetAsync(h->ids.p, 0xff, (size_t)npad * 8, h->stream));  // -1
  ANR_HIP(hipMemsetAsync(h->n2.p, 0, (size_t)npad * 8, h->stream));
  if (h->n_alive > 0) {
    std::vector<int64_t> offs(2 * nl);
    for (int l = 0; l < nl; ++l) {
      offs[l] = h->list_off[l];
      offs[nl + l] = seg_start[l];
    }
    ANR_HIP(hipMemcpyAsync(h->off_d.p, offs.data(), (size_t)2 * nl * 8, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_ivf_gather, dim3((unsigned)ceil_div(h->n_alive, 4)), dim3(256), 0, h->stream, h->xall.p, dim,
                       h->skeys2.p, h->svals2.p, h->n_alive, h->off_d.p, h->off_d.p + nl, h->xs.p, h->x16.p, h->ids.p,
                       h->n2.p);
    ANR_HIP(hipGetLastError());
  }
  ANR_HIP(hipStreamSynchronize(h->stream));
  return ANR_OK;
}

int reassign_all(anr_ivf *h) {
  if (h->pq) return reencode_all(h);
  if (h->n_all > 0) ANR_TRY(assign_rows(h, h->xall.p, h->xnrm.p, h->n_all, h->assign.p));
  h->dirty = true;
  return ANR_OK;
}

// the list-ordered copy is rebuilt once before it is read (adds, removals and centroid changes only mark it stale, so a
// load that adds chunk by chunk costs one rebuild)
int ensure_built(anr_ivf *h) {
  if (!h->dirty) return ANR_OK;
  ANR_TRY(h->pq ? rebuild_pq(h) : rebuild(h));
  h->dirty = false;
  return ANR_OK;
}

int grow_all(anr_ivf *h, int64_t n_new) {
  const int64_t need = h->n_all + n_new;
  if (need <= h->xall.cap / h->dim && h->xall.p) return ANR_OK;
  const int64_t cap = std::max<int64_t>(need, h->n_all + h->n_all / 2);
  DevBuf<float> nx, nn;
  DevBuf<int32_t> na;
  DevBuf<uint8_t> nal;
  ANR_TRY(nx.alloc(cap * h->dim, "ivf"));
  ANR_TRY(nn.alloc(cap, "ivf"));
  ANR_TRY(na.alloc(cap, "ivf"));
  ANR_TRY(nal.alloc(cap, "ivf"));
  if (h->n_all > 0) {
    ANR_HIP(hipMemcpyAsync(nx.p, h->xall.p, (size_t)h->n_all * h->dim * 4, hipMemcpyDeviceToDevice, h->stream));
    ANR_HIP(hipMemcpyAsync(nn.p, h->xnrm.p, (size_t)h->n_all * 4, hipMemcpyDeviceToDevice, h->stream));
    ANR_HIP(hipMemcpyAsync(na.p, h->assign.p, (size_t)h->n_all * 4, hipMemcpyDeviceToDevice, h->stream));
    ANR_HIP(hipMemcpyAsync(nal.p, h->alive_d.p, (size_t)h->n_all, hipMemcpyDeviceToDevice, h->stream));
    ANR_HIP(hipStreamSynchronize(h->stream));
  }
  h->xall = std::move(nx);  // the old blocks are freed here
  h->xnrm = std::move(nn);
  h->assign = std::move(na);
  h->alive_d = std::move(nal);
  return ANR_OK;
}

int add_impl(anr_ivf *h, const float *x, int64_t n, bool host) {
  if (h->pq) return add_pq(h, x, n, host);
  if (!h->trained) return fail(ANR_ESTATE, "anr_ivf_add: the index has no centroids (train or set_centroids first)");
  if (n == 0) return ANR_OK;
  // padded list rows are addressed with int32 in the search
  if (h->n_all + n + (int64_t)kTile * h->nlist > 0x7fffffffll) return fail(ANR_EINVAL, "anr_ivf_add: too many rows");
  ANR_TRY(grow_all(h, n));
  float *dst = h->xall.p + h->n_all * h->dim;
  float *dn = h->xnrm.p + h->n_all;
  ANR_TRY(stage_rows(h, x, n, host, dst, dn, h->add_raw != 0));
  ANR_TRY(assign_rows(h, dst, dn, n, h->assign.p + h->n_all));
  ANR_HIP(hipMemsetAsync(h->alive_d.p + h->n_all, 1, (size_t)n, h->stream));
  std::vector<float> nr(n);
  ANR_HIP(hipMemcpyAsync(nr.data(), dn, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
  ANR_HIP(hipStreamSynchronize(h->stream));
  for (float v : nr) h->max_norm = std::max(h->max_norm, v);
  h->alive.resize(h->n_all + n, 1);
  h->n_all += n;
  h->n_alive += n;
  h->dirty = true;
  return ANR_OK;
}

// Lloyd's iterations over m preprocessed rows at h->xall-like buffer x (norms xn), from the current centroids
int lloyd(anr_ivf *h, const float *x, const float *xn, int64_t m, int niter, DevBuf<int32_t> &asg) {
  const int nl = h->nlist;
  ANR_TRY(need(asg, m));
  ANR_TRY(need(h->seg, 2 * nl));
  std::vector<int64_t> cnt, seg(2 * nl);
  for (int it = 0; it < niter; ++it) {
    ANR_TRY(assign_rows(h, x, xn, m, asg.p));
    ANR_TRY(sort_by_list(h, asg.p, nullptr, m, cnt));
    int64_t s = 0;
    for (int l = 0; l < nl; ++l) {
      seg[2 * l] = s;
      seg[2 * l + 1] = cnt[l];
      s += cnt[l];
    }
    // empty lists take the second half of the largest one (see the file comment)
    for (int j = 0; j < nl; ++j) {
      if (seg[2 * j + 1] != 0) continue;
      int b = 0;
      for (int l = 1; l < nl; ++l)
        if (seg[2 * l + 1] > seg[2 * b + 1]) b = l;
      const int64_t cb = seg[2 * b + 1];
      if (cb < 2) break;
      const int64_t keep = cb - cb / 2;
      seg[2 * j] = seg[2 * b] + keep;
      seg[2 * j + 1] = cb / 2;
      seg[2 * b + 1] = keep;
    }
    ANR_HIP(hipMemcpyAsync(h->seg.p, seg.data(), (size_t)2 * nl * 8, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_ivf_seg_mean, dim3((unsigned)nl), dim3(256), 0, h->stream, x, h->dim, h->svals2.p, h->seg.p,
                       h->cent.p);
    ANR_HIP(hipGetLastError());
    if (h->spherical) {  // spherical k-means: every centroid back to unit norm (zero stays zero), as the rows are normalised
      hipLaunchKernelGGL(k_ivf_prep, dim3((unsigned)ceil_div(nl, 4)), dim3(256), 0, h->stream, h->cent.p, (int64_t)nl,
                         h->dim, 1, h->cent.p, h->cnrm.p);
      ANR_HIP(hipGetLastError());
    }
    ANR_TRY(update_cstats(h));
  }
  return ANR_OK;
}

int alloc_centroids(anr_ivf *h) {
  ANR_TRY(need(h->cent, (int64_t)h->nlist * h->dim));
  ANR_TRY(need(h->cn2, h->nlist));
  ANR_TRY(need(h->cnrm, h->nlist));
  return ANR_OK;
}

int search_impl(anr_ivf *h, const float *qin, bool host, int64_t nq, int k, int nprobe, float *D, int64_t *I) {
  if (h->pq) return search_pq(h, qin, host, nq, k, nprobe, D, I);
  const int dim = h->dim, nl = h->nlist, l2 = h->metric == ANR_METRIC_L2;
  if (k <= 0 || k > kIvfMaxK) return fail(ANR_EINVAL, "k must be in 1..%d (got %d)", kIvfMaxK, k);
  if (nprobe <= 0) return fail(ANR_EINVAL, "nprobe must be positive (got %d)", nprobe);
  if (!h->trained) return fail(ANR_ESTATE, "anr_ivf_search: the index has no centroids");
  nprobe = std::min(nprobe, nl);
  h->last_nq = nq;
  h->last_exhaust = 0;
  if (nq == 0) return ANR_OK;
  ANR_TRY(ensure_built(h));
  ANR_TRY(need(h->qbuf, nq * dim));
  ANR_TRY(need(h->qnrm, nq));
  ANR_TRY(stage_rows(h, qin, nq, host, h->qbuf.p, h->qnrm.p));
  // coarse
  ANR_TRY(need(h->cs, nq * nl));
  ANR_TRY(need(h->probe, nq * nprobe));
  hipLaunchKernelGGL(k_ivf_coarse, dim3((unsigned)nq, (unsigned)ceil_div(nl, 64)), dim3(256), 0, h->stream, h->qbuf.p, dim,
                     h->cent.p, nl, l2, h->cs.p);
  int np2 = 2;
  while (np2 < nl) np2 <<= 1;
  const int lds = np2 * 12;
  ANR_TRY(ensure_dynamic_lds((const void *)k_ivf_topp, kIvfMaxNlist * 12));
  hipLaunchKernelGGL(k_ivf_topp, dim3((unsigned)nq), dim3(1024), lds, h->stream, h->cs.p, nl, np2, nprobe, h->probe.p);
  ANR_HIP(hipGetLastError());
  std::vector<int32_t> probe(nq * nprobe);
  std::vector<float> qn(nq);
  ANR_HIP(hipMemcpyAsync(probe.data(), h->probe.p, probe.size() * 4, hipMemcpyDeviceToHost, h->stream));
  ANR_HIP(hipMemcpyAsync(qn.data(), h->qnrm.p, (size_t)nq * 4, hipMemcpyDeviceToHost, h->stream));
  ANR_HIP(hipStreamSynchronize(h->stream));

  // (query, list) pairs grouped by list; per query its probed segments back to back
  std::vector<int64_t> cbase(nq), ctot(nq, 0);
  std::vector<std::vector<std::pair<int32_t, int64_t>>> bylist(nl);
  int64_t total = 0;
  for (int64_t qi = 0; qi < nq; ++qi) {
    cbase[qi] = total;
    for (int j = 0; j < nprobe; ++j) {
      const int l = probe[qi * nprobe + j];
      const int64_t len = h->list_off[l + 1] - h->list_off[l];
      if (len == 0) continue;
      bylist[l].push_back({(int32_t)qi, ctot[qi]});
      ctot[qi] += len;
    }
    total += ctot[qi];
  }
  std::vector<int32_t> eq;
  std::vector<int64_t> eoff;
  std::vector<ProbeItem> items;
  for (int l = 0; l < nl; ++l) {
    if (bylist[l].empty()) continue;
    const int32_t e0 = (int32_t)eq.size();
    for (auto &p : bylist[l]) {
      eq.push_back(p.first);
      eoff.push_back(p.second);
    }
    const int32_t e1 = (int32_t)eq.size();
    for (int64_t t = h->list_off[l]; t < h->list_off[l + 1]; t += kTile) items.push_back({t, t - h->list_off[l], e0, e1});
  }
  // certificate bound per query (see the file comment): f16 rounding of the rows + float32 accumulation (+ the L2 terms)
  std::vector<float> qb(nq);
  const double u = std::ldexp(1.0, -24), M = h->max_norm;
  for (int64_t qi = 0; qi < nq; ++qi) {
    const double Q = qn[qi];
    const double bdot = Q * (M * (std::ldexp(1.0, -11) + (dim + 16) * u) * 1.05 + std::sqrt((double)dim) * std::ldexp(1.0, -24));
    const double b = l2 ? 2.0 * bdot + 8.0 * (M + Q) * (M + Q) * u : bdot + 2.0 * Q * M * u;
    qb[qi] = (float)(b * 1.25 + 1e-30);
  }
  // K': the flat index's f16 ladder starts near 2k; an image that cannot hold the rows (|x_i| > 65504) is never trusted
  int kp = std::max(2 * k, k + 64);
  kp = std::min(kp, kSelCap);
  const bool trust16 = h->max_norm < 60000.0f;

  ANR_TRY(need(h->cbase, nq));
  ANR_TRY(need(h->ctot, nq));
  ANR_TRY(need(h->qbound, nq));
  ANR_TRY(need(h->ckey, std::max<int64_t>(total, 1)));
  ANR_TRY(need(h->cpos, std::max<int64_t>(total, 1)));
  ANR_TRY(need(h->eq, std::max<int64_t>(eq.size(), 1)));
  ANR_TRY(need(h->eoff, std::max<int64_t>(eoff.size(), 1)));
  ANR_TRY(need(h->items, std::max<int64_t>(items.size(), 1)));
  ANR_TRY(need(h->qn2, nq));
  ANR_TRY(need(h->Dd, nq * k));
  ANR_TRY(need(h->Id, nq * k));
  ANR_TRY(need(h->failq, nq));
  ANR_TRY(need(h->qlist, nq));
  std::vector<float> qn2(nq);
  for (int64_t qi = 0; qi < nq; ++qi) qn2[qi] = (float)((double)qn[qi] * qn[qi]);
  ANR_HIP(hipMemcpyAsync(h->cbase.p, cbase.data(), nq * 8, hipMemcpyHostToDevice, h->stream));
  ANR_HIP(hipMemcpyAsync(h->ctot.p, ctot.data(), nq * 8, hipMemcpyHostToDevice, h->stream));
  ANR_HIP(hipMemcpyAsync(h->qbound.p, qb.data(), nq * 4, hipMemcpyHostToDevice, h->stream));
  ANR_HIP(hipMemcpyAsync(h->qn2.p, qn2.data(), nq * 4, hipMemcpyHostToDevice, h->stream));
  if (!items.empty()) {
    ANR_HIP(hipMemcpyAsync(h->eq.p, eq.data(), eq.size() * 4, hipMemcpyHostToDevice, h->stream));
    ANR_HIP(hipMemcpyAsync(h->eoff.p, eoff.data(), eoff.size() * 8, hipMemcpyHostToDevice, h->stream));
    ANR_HIP(hipMemcpyAsync(h->items.p, items.data(), items.size() * sizeof(ProbeItem), hipMemcpyHostToDevice, h->stream));
    const int plds = kTile * (dim / 2 + 1) * 4;
    ANR_TRY(ensure_dynamic_lds((const void *)k_ivf_probe, kTile * (kIvfMaxDim / 2 + 1) * 4));
    hipLaunchKernelGGL(k_ivf_probe, dim3((unsigned)items.size()), dim3(256), plds, h->stream, h->x16.p, h->ids.p, h->n2.p,
                       dim, h->qbuf.p, h->qn2.p, l2, h->items.p, h->eq.p, h->eoff.p, h->cbase.p, h->ckey.p, h->cpos.p);
    ANR_HIP(hipGetLastError());
  }
  std::vector<int32_t> failed(nq, 1);
  if (trust16) {
    hipLaunchKernelGGL(k_ivf_select, dim3((unsigned)nq), dim3(1024), 0, h->stream, h->ckey.p, h->cpos.p, h->cbase.p,
                       h->ctot.p, h->xs.p, h->ids.p, h->qbuf.p, dim, l2, k, kp, h->qbound.p, h->Dd.p, h->Id.p, h->failq.p);
    ANR_HIP(hipGetLastError());
    ANR_HIP(hipMemcpyAsync(failed.data(), h->failq.p, nq * 4, hipMemcpyDeviceToHost, h->stream));
  }
  ANR_HIP(hipStreamSynchronize(h->stream));
  std::vector<int32_t> ql;
  for (int64_t qi = 0; qi < nq; ++qi)
    if (failed[qi]) ql.push_back((int32_t)qi);
  h->last_exhaust = (int64_t)ql.size();
  if (!ql.empty()) {
    ANR_HIP(hipMemcpyAsync(h->qlist.p, ql.data(), ql.size() * 4, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_ivf_exhaust, dim3((unsigned)ql.size()), dim3(1024), 0, h->stream, h->qlist.p, h->ckey.p, h->cpos.p,
                       h->cbase.p, h->ctot.p, h->xs.p, h->ids.p, h->qbuf.p, dim, l2, k, h->Dd.p, h->Id.p);
    ANR_HIP(hipGetLastError());
  }
  if (D) ANR_HIP(hipMemcpyAsync(D, h->Dd.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost, h->stream));
  if (I) ANR_HIP(hipMemcpyAsync(I, h->Id.p, (size_t)nq * k * 8, hipMemcpyDeviceToHost, h->stream));
  ANR_HIP(hipStreamSynchronize(h->stream));
  return ANR_OK;
}


// ---------------------------------------------------------------------------------------------------------------
// product quantiser, host side

template <typename T>
int exact_alloc(DevBuf<T> &b, int64_t n) {  // persistent buffers of a PQ handle hold what they store, no growth slack
  if (b.cap != n) b.release();
  return b.alloc(n, "ivf");
}

// device scratch of one encoding pass, released when the pass ends
struct PqScratch {
  DevBuf<float> x, xn, res, rn;
  DevBuf<int32_t> asg, c32;
  DevBuf<uint8_t> c8;
};

// |entry|^2 and |entry| of every codebook entry, and per sub-space the largest norm (the assignment's error bound)
int update_pq_stats(anr_ivf *h) {
  const int nc = h->m * 256;
  hipLaunchKernelGGL(k_ivf_cstat, dim3((unsigned)ceil_div(nc, 4)), dim3(256), 0, h->stream, h->cb.p, nc, h->dsub,
                     h->cbn2.p, h->cbnrm.p);
  ANR_HIP(hipGetLastError());
  std::vector<float> nr(nc), mx(h->m, 0.0f);
  ANR_HIP(hipMemcpyAsync(nr.data(), h->cbnrm.p, (size_t)nc * 4, hipMemcpyDeviceToHost, h->stream));
  ANR_HIP(hipStreamSynchronize(h->stream));
  for (int e = 0; e < nc; ++e) mx[e >> 8] = std::max(mx[e >> 8], nr[e]);
  for (float &v : mx) v *= 1.0001f;
  ANR_HIP(hipMemcpyAsync(h->cbmax.p, mx.data(), (size_t)h->m * 4, hipMemcpyHostToDevice, h->stream));
  return ANR_OK;
}

// code of every sub-vector of n residual rows res (sub-vector norms rn [n][m]) -> out [n][m]: float32 tiles, float64
// re-check of near ties
int pq_assign(anr_ivf *h, const float *res, const float *rn, int64_t n, int32_t *out) {
  if (n == 0) return ANR_OK;
  const int64_t nm = n * h->m;
  ANR_TRY(need(h->fix, nm));
  ANR_TRY(need(h->nfix, 1));
  ANR_HIP(hipMemsetAsync(h->nfix.p, 0, 4, h->stream));
  hipLaunchKernelGGL(k_pq_assign, dim3((unsigned)ceil_div(n, 64), (unsigned)h->m), dim3(256), 0, h->stream, res, n, h->dim,
                     h->dsub, h->m, h->cb.p, h->cbn2.p, rn, h->cbmax.p, out, h->fix.p, h->nfix.p);
  ANR_HIP(hipGetLastError());
  int32_t nf = 0;
  ANR_HIP(hipMemcpyAsync(&nf, h->nfix.p, 4, hipMemcpyDeviceToHost, h->stream));
  ANR_HIP(hipStreamSynchronize(h->stream));
  if (nf > 0) {
    hipLaunchKernelGGL(k_pq_assign_fix, dim3((unsigned)nf), dim3(256), 0, h->stream, res, h->dsub, h->m, h->cb.p,
                       h->fix.p, h->nfix.p, out);
    ANR_HIP(hipGetLastError());
  }
  return ANR_OK;
}

// residuals of n preprocessed rows x (norms xn) against their coarse lists (written to asg) and the norms of their
// sub-vectors, into sc.res / sc.rn
int pq_residuals(anr_ivf *h, const float *x, const float *xn, int64_t n, int32_t *asg, PqScratch &sc) {
  ANR_TRY(need(sc.res, n * h->dim));
  ANR_TRY(need(sc.rn, n * h->m));
  ANR_TRY(assign_rows(h, x, xn, n, asg));
  hipLaunchKernelGGL(k_pq_residual, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, h->stream, x, n, h->dim, h->cent.p, asg,
                     sc.res.p);
  ANR_HIP(hipGetLastError());
  // the residual rows are [n * m][dsub]: k_ivf_prep without normalisation leaves them as they are and gives the norms
  hipLaunchKernelGGL(k_ivf_prep, dim3((unsigned)ceil_div(n * h->m, 4)), dim3(256), 0, h->stream, sc.res.p, n * h->m,
                     h->dsub, 0, sc.res.p, sc.rn.p);
  ANR_HIP(hipGetLastError());
  return ANR_OK;
}

// Lloyd's iterations of all m sub-space k-means at once (256 entries each, L2, never spherical) over n residual rows,
// from the current codebooks; means and the empty-entry split rule as in lloyd()
int pq_lloyd(anr_ivf *h, const float *res, const float *rn, int64_t n, int niter) {
  const int64_t nm = n * h->m;
  const int nc = h->m * 256;
  DevBuf<int32_t> asg;
  DevBuf<int64_t> sg;
  int r = need(asg, nm);
  if (r == ANR_OK) r = need(sg, 2 * nc);
  if (r == ANR_OK) r = need(h->skeys, nm);
  if (r == ANR_OK) r = need(h->skeys2, nm);
  if (r == ANR_OK) r = need(h->svals, nm);
  if (r == ANR_OK) r = need(h->svals2, nm);
  if (r == ANR_OK) r = need(h->stemp, (int64_t)radix_sort_temp_bytes(nm));
  if (r == ANR_OK) r = need(h->counts, nc);
  std::vector<int32_t> cnt(nc);
  std::vector<int64_t> seg(2 * nc);
  for (int it = 0; it < niter && r == ANR_OK; ++it) {
    r = pq_assign(h, res, rn, n, asg.p);
    if (r != ANR_OK) break;
    if (hipMemsetAsync(h->counts.p, 0, (size_t)nc * 4, h->stream) != hipSuccess) r = fail(ANR_EHIP, "pq: memset failed");
    if (r != ANR_OK) break;
    hipLaunchKernelGGL(k_pq_keys, dim3((unsigned)ceil_div(nm, 256)), dim3(256), 0, h->stream, asg.p, n, h->m, h->skeys.p,
                       h->svals.p, h->counts.p);
    r = radix_sort_pairs_u64(h->stemp.p, h->skeys.p, h->skeys2.p, h->svals.p, h->svals2.p, nm, false, h->stream);
    if (r != ANR_OK) break;
    if (hipMemcpyAsync(cnt.data(), h->counts.p, (size_t)nc * 4, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess) {
      r = fail(ANR_EHIP, "pq: k-means step failed");
      break;
    }
    int64_t s = 0;
    for (int e = 0; e < nc; ++e) {
      seg[2 * e] = s;
      seg[2 * e + 1] = cnt[e];
      s += cnt[e];
    }
    for (int j = 0; j < h->m; ++j) {  // per sub-space, the split rule of lloyd()
      int64_t *sj = seg.data() + (int64_t)2 * 256 * j;
      for (int c = 0; c < 256; ++c) {
        if (sj[2 * c + 1] != 0) continue;
        int b = 0;
        for (int l = 1; l < 256; ++l)
          if (sj[2 * l + 1] > sj[2 * b + 1]) b = l;
        const int64_t cb = sj[2 * b + 1];
        if (cb < 2) break;
        const int64_t keep = cb - cb / 2;
        sj[2 * c] = sj[2 * b] + keep;
        sj[2 * c + 1] = cb / 2;
        sj[2 * b + 1] = keep;
      }
    }
    if (hipMemcpyAsync(sg.p, seg.data(), (size_t)2 * nc * 8, hipMemcpyHostToDevice, h->stream) != hipSuccess) {
      r = fail(ANR_EHIP, "pq: copy failed");
      break;
    }
    hipLaunchKernelGGL(k_pq_seg_mean, dim3((unsigned)nc), dim3(64), 0, h->stream, res, h->dim, h->dsub, h->svals2.p, sg.p,
                       h->cb.p);
    if (hipGetLastError() != hipSuccess) r = fail(ANR_EHIP, "pq: launch failed");
    if (r == ANR_OK) r = update_pq_stats(h);
  }
  return r;
}

// preprocess (raw: as given), assign, encode n rows at src (host or device), kPqChunk rows at a time; per row its list
// and codes (and, when rows_out is given, the preprocessed row) go to the host arrays
int pq_encode(anr_ivf *h, const float *src, bool host, int64_t n, bool raw, float *rows_out, int32_t *asg_out,
              uint8_t *codes_out, float *max_norm) {
  PqScratch sc;
  const int dim = h->dim, m = h->m;
  int r = ANR_OK;
  std::vector<float> nr;
  for (int64_t s = 0; s < n && r == ANR_OK; s += kPqChunk) {
    const int64_t c = std::min<int64_t>(kPqChunk, n - s);
    r = need(sc.x, c * dim);
    if (r == ANR_OK) r = need(sc.xn, c);
    if (r == ANR_OK) r = need(sc.asg, c);
    if (r == ANR_OK) r = need(sc.c32, c * m);
    if (r == ANR_OK) r = need(sc.c8, c * m);
    if (r == ANR_OK) r = stage_rows(h, src + s * dim, c, host, sc.x.p, sc.xn.p, raw);
    if (r == ANR_OK) r = pq_residuals(h, sc.x.p, sc.xn.p, c, sc.asg.p, sc);
    if (r == ANR_OK) r = pq_assign(h, sc.res.p, sc.rn.p, c, sc.c32.p);
    if (r != ANR_OK) break;
    hipLaunchKernelGGL(k_pq_pack, dim3((unsigned)ceil_div(c * m, 256)), dim3(256), 0, h->stream, sc.c32.p, c * m, sc.c8.p);
    bool ok = hipGetLastError() == hipSuccess;
    ok = ok && hipMemcpyAsync(asg_out + s, sc.asg.p, (size_t)c * 4, hipMemcpyDeviceToHost, h->stream) == hipSuccess;
    ok = ok && hipMemcpyAsync(codes_out + s * m, sc.c8.p, (size_t)c * m, hipMemcpyDeviceToHost, h->stream) == hipSuccess;
    if (rows_out)
      ok = ok && hipMemcpyAsync(rows_out + s * dim, sc.x.p, (size_t)c * dim * 4, hipMemcpyDeviceToHost, h->stream) ==
                     hipSuccess;
    if (max_norm) {
      nr.resize(c);
      ok = ok && hipMemcpyAsync(nr.data(), sc.xn.p, (size_t)c * 4, hipMemcpyDeviceToHost, h->stream) == hipSuccess;
    }
    ok = ok && hipStreamSynchronize(h->stream) == hipSuccess;
    if (!ok) r = fail(ANR_EHIP, "pq: encoding failed");
    if (max_norm)
      for (float v : nr) *max_norm = std::max(*max_norm, v);
  }
  return r;
}

// every stored row again (after a change of the centroids or codebooks); without codebooks there is nothing to encode
int reencode_all(anr_ivf *h) {
  h->dirty = true;
  if (!h->pq_ready || h->n_all == 0) return ANR_OK;
  return pq_encode(h, h->xh.data(), true, h->n_all, true, nullptr, h->assign_h.data(), h->codes_h.data(), nullptr);
}

int add_pq(anr_ivf *h, const float *x, int64_t n, bool host) {
  if (!h->trained || !h->pq_ready)
    return fail(ANR_ESTATE, "anr_ivf_add: the index has no centroids or codebooks (train or set them first)");
  if (n == 0) return ANR_OK;
  if (h->n_all + n + (int64_t)kPqTile * h->nlist > 0x7fffffffll) return fail(ANR_EINVAL, "anr_ivf_add: too many rows");
  const int64_t n0 = h->n_all;
  h->xh.resize((size_t)(n0 + n) * h->dim);
  h->assign_h.resize(n0 + n);
  h->codes_h.resize((size_t)(n0 + n) * h->m);
  float mx = h->max_norm;
  const int r = pq_encode(h, x, host, n, h->add_raw != 0, h->xh.data() + n0 * h->dim, h->assign_h.data() + n0,
                          h->codes_h.data() + n0 * h->m, &mx);
  if (r != ANR_OK) {  // the index stays as it was
    h->xh.resize((size_t)n0 * h->dim);
    h->assign_h.resize(n0);
    h->codes_h.resize((size_t)n0 * h->m);
    return r;
  }
  h->max_norm = mx;
  h->alive.resize(n0 + n, 1);
  h->n_all += n;
  h->n_alive += n;
  h->dirty = true;
  return ANR_OK;
}

// the list-ordered code tiles and ids, from the host's lists / alive flags / codes (device scratch released after)
int rebuild_pq(anr_ivf *h) {
  const int nl = h->nlist;
  h->list_cnt.assign(nl, 0);
  h->list_off.assign(nl + 1, 0);
  DevBuf<int32_t> asg;
  DevBuf<uint8_t> al, c8;
  int r = ANR_OK;
  std::vector<int64_t> seg_start(nl);
  if (h->n_all > 0) {
    r = need(asg, h->n_all);
    if (r == ANR_OK) r = need(al, h->n_all);
    if (r == ANR_OK && (hipMemcpyAsync(asg.p, h->assign_h.data(), (size_t)h->n_all * 4, hipMemcpyHostToDevice,
                                       h->stream) != hipSuccess ||
                        hipMemcpyAsync(al.p, h->alive.data(), (size_t)h->n_all, hipMemcpyHostToDevice, h->stream) !=
                            hipSuccess))
      r = fail(ANR_EHIP, "pq: copy failed");
    if (r == ANR_OK) r = sort_by_list(h, asg.p, al.p, h->n_all, h->list_cnt);
  }
  int64_t s = 0;
  for (int l = 0; l < nl; ++l) {
    seg_start[l] = s;
    s += h->list_cnt[l];
    h->list_off[l + 1] = h->list_off[l] + round_up(h->list_cnt[l], kPqTile);
  }
  const int64_t npad = std::max<int64_t>(h->list_off[nl], kPqTile);
  if (r == ANR_OK) r = exact_alloc(h->lcodes, npad * h->m4);
  if (r == ANR_OK) r = exact_alloc(h->ids, npad);
  if (r == ANR_OK) r = need(h->off_d, 2 * nl);
  if (r == ANR_OK && (hipMemsetAsync(h->lcodes.p, 0, (size_t)npad * h->m4 * 4, h->stream) != hipSuccess ||
                      hipMemsetAsync(h->ids.p, 0xff, (size_t)npad * 8, h->stream) != hipSuccess))
    r = fail(ANR_EHIP, "pq: memset failed");
  if (r == ANR_OK && h->n_alive > 0) {
    std::vector<int64_t> offs(2 * nl);
    for (int l = 0; l < nl; ++l) {
      offs[l] = h->list_off[l];
      offs[nl + l] = seg_start[l];
    }
    r = need(c8, h->n_all * h->m);
    if (r == ANR_OK &&
        (hipMemcpyAsync(c8.p, h->codes_h.data(), (size_t)h->n_all * h->m, hipMemcpyHostToDevice, h->stream) !=
             hipSuccess ||
         hipMemcpyAsync(h->off_d.p, offs.data(), (size_t)2 * nl * 8, hipMemcpyHostToDevice, h->stream) != hipSuccess))
      r = fail(ANR_EHIP, "pq: copy failed");
    if (r == ANR_OK) {
      hipLaunchKernelGGL(k_pq_gather, dim3((unsigned)ceil_div(h->n_alive, 256)), dim3(256), 0, h->stream, c8.p, h->m,
                         h->m4, h->skeys2.p, h->svals2.p, h->n_alive, h->off_d.p, h->off_d.p + nl,
                         reinterpret_cast<uint8_t *>(h->lcodes.p), h->ids.p);
      if (hipGetLastError() != hipSuccess) r = fail(ANR_EHIP, "pq: launch failed");
    }
  }
  if (hipStreamSynchronize(h->stream) != hipSuccess && r == ANR_OK) r = fail(ANR_EHIP, "pq: rebuild failed");
  for (auto *b : {&h->skeys, &h->skeys2}) b->release();
  for (auto *b : {&h->svals, &h->svals2}) b->release();
  h->stemp.release();
  h->off_d.release();
  return r;
}

// ADC search: coarse probing as search_impl, then the probed lists' code tiles scored through the LUT, top-k by
// (key desc, id asc)
int search_pq(anr_ivf *h, const float *qin, bool host, int64_t nq, int k, int nprobe, float *D, int64_t *I) {
  const int dim = h->dim, nl = h->nlist, l2 = h->metric == ANR_METRIC_L2;
  if (k <= 0 || k > kIvfMaxK) return fail(ANR_EINVAL, "k must be in 1..%d (got %d)", kIvfMaxK, k);
  if (nprobe <= 0) return fail(ANR_EINVAL, "nprobe must be positive (got %d)", nprobe);
  if (!h->trained || !h->pq_ready) return fail(ANR_ESTATE, "anr_ivf_search: the index has no centroids or codebooks");
  nprobe = std::min(nprobe, nl);
  h->last_nq = nq;
  h->last_exhaust = 0;
  if (nq == 0) return ANR_OK;
  ANR_TRY(ensure_built(h));
  ANR_TRY(need(h->qbuf, nq * dim));
  ANR_TRY(need(h->qnrm, nq));
  ANR_TRY(stage_rows(h, qin, nq, host, h->qbuf.p, h->qnrm.p));
  ANR_TRY(need(h->cs, nq * nl));
  ANR_TRY(need(h->probe, nq * nprobe));
  hipLaunchKernelGGL(k_ivf_coarse, dim3((unsigned)nq, (unsigned)ceil_div(nl, 64)), dim3(256), 0, h->stream, h->qbuf.p, dim,
                     h->cent.p, nl, l2, h->cs.p);
  int np2 = 2;
  while (np2 < nl) np2 <<= 1;
  ANR_TRY(ensure_dynamic_lds((const void *)k_ivf_topp, kIvfMaxNlist * 12));
  hipLaunchKernelGGL(k_ivf_topp, dim3((unsigned)nq), dim3(1024), np2 * 12, h->stream, h->cs.p, nl, np2, nprobe, h->probe.p);
  ANR_HIP(hipGetLastError());
  const int mp = 4 * h->m4;
  if (!l2) {  // the queries' inner-product LUTs, while the host waits for the probe lists
    ANR_TRY(need(h->lut, nq * mp * 256));
    hipLaunchKernelGGL(k_pq_lut, dim3((unsigned)nq, (unsigned)mp), dim3(256), 0, h->stream, h->qbuf.p, dim, h->dsub, h->m,
                       h->cb.p, h->lut.p);
    ANR_HIP(hipGetLastError());
  }
  std::vector<int32_t> probe(nq * nprobe);
  ANR_HIP(hipMemcpyAsync(probe.data(), h->probe.p, probe.size() * 4, hipMemcpyDeviceToHost, h->stream));
  ANR_HIP(hipStreamSynchronize(h->stream));
  std::vector<int64_t> cbase(nq), ctot(nq, 0);
  std::vector<PqItem> items;
  int64_t total = 0;
  for (int64_t qi = 0; qi < nq; ++qi) {
    cbase[qi] = total;
    for (int j = 0; j < nprobe; ++j) {
      const int l = probe[qi * nprobe + j];
      const int64_t len = h->list_off[l + 1] - h->list_off[l], nt = len / kPqTile;
      for (int64_t t = 0; t < nt; t += kPqItemTiles)
        items.push_back({h->list_off[l] / kPqTile + t, total + ctot[qi] + t * kPqTile, (int32_t)qi, (int32_t)l,
                         (int32_t)std::min<int64_t>(kPqItemTiles, nt - t)});
      ctot[qi] += len;
    }
    total += ctot[qi];
  }
  ANR_TRY(need(h->cbase, nq));
  ANR_TRY(need(h->ctot, nq));
  ANR_TRY(need(h->ckey, std::max<int64_t>(total, 1)));
  ANR_TRY(need(h->cpos, std::max<int64_t>(total, 1)));
  ANR_TRY(need(h->pitems, std::max<int64_t>(items.size(), 1)));
  ANR_TRY(need(h->Dd, nq * k));
  ANR_TRY(need(h->Id, nq * k));
  ANR_HIP(hipMemcpyAsync(h->cbase.p, cbase.data(), nq * 8, hipMemcpyHostToDevice, h->stream));
  ANR_HIP(hipMemcpyAsync(h->ctot.p, ctot.data(), nq * 8, hipMemcpyHostToDevice, h->stream));
  if (!items.empty()) {
    ANR_HIP(hipMemcpyAsync(h->pitems.p, items.data(), items.size() * sizeof(PqItem), hipMemcpyHostToDevice, h->stream));
    const int lds = mp * 256 * 4 + (l2 ? dim * 4 : 0);
    const void *kern = l2 ? (const void *)k_pq_scan<1> : (const void *)k_pq_scan<0>;
    ANR_TRY(ensure_dynamic_lds(kern, kPqMaxM * 256 * 4 + kIvfMaxDim * 4));
    if (l2)
      hipLaunchKernelGGL(k_pq_scan<1>, dim3((unsigned)items.size()), dim3(256), lds, h->stream, h->pitems.p, h->lcodes.p,
                         h->ids.p, h->m4, h->dsub, dim, h->lut.p, h->qbuf.p, h->cent.p, h->cb.p, h->m, h->cs.p, nl,
                         h->ckey.p, h->cpos.p);
    else
      hipLaunchKernelGGL(k_pq_scan<0>, dim3((unsigned)items.size()), dim3(256), lds, h->stream, h->pitems.p, h->lcodes.p,
                         h->ids.p, h->m4, h->dsub, dim, h->lut.p, h->qbuf.p, h->cent.p, h->cb.p, h->m, h->cs.p, nl,
                         h->ckey.p, h->cpos.p);
    ANR_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_pq_select, dim3((unsigned)nq), dim3(1024), 0, h->stream, h->ckey.p, h->cpos.p, h->cbase.p, h->ctot.p,
                     h->ids.p, l2, k, h->Dd.p, h->Id.p);
  ANR_HIP(hipGetLastError());
  if (D) ANR_HIP(hipMemcpyAsync(D, h->Dd.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost, h->stream));
  if (I) ANR_HIP(hipMemcpyAsync(I, h->Id.p, (size_t)nq * k * 8, hipMemcpyDeviceToHost, h->stream));
  ANR_HIP(hipStreamSynchronize(h->stream));
  return ANR_OK;
}

// the PQ's training rows: the rows `rows` of x_host (preprocessed on the device), their residuals, m k-means of
// kPqNiter iterations from the sub-vectors of the first 256 rows
int train_pq(anr_ivf *h, const float *x_host, const std::vector<int64_t> &rows) {
  const int64_t n = (int64_t)rows.size();
  const int dim = h->dim;
  std::vector<float> xt((size_t)n * dim);
  for (int64_t i = 0; i < n; ++i) std::memcpy(&xt[i * dim], x_host + rows[i] * dim, (size_t)dim * 4);
  PqScratch sc;
  int r = need(sc.x, n * dim);
  if (r == ANR_OK) r = need(sc.xn, n);
  if (r == ANR_OK) r = need(sc.asg, n);
  if (r == ANR_OK) r = stage_rows(h, xt.data(), n, true, sc.x.p, sc.xn.p);
  if (r == ANR_OK) r = pq_residuals(h, sc.x.p, sc.xn.p, n, sc.asg.p, sc);
  // codebook entry c of sub-space j = sub-vector j of residual row c: [c][j][dsub] -> [j][c][dsub]
  for (int j = 0; j < h->m && r == ANR_OK; ++j)
    if (hipMemcpy2DAsync(h->cb.p + (int64_t)j * 256 * h->dsub, (size_t)h->dsub * 4, sc.res.p + (int64_t)j * h->dsub,
                         (size_t)dim * 4, (size_t)h->dsub * 4, 256, hipMemcpyDeviceToDevice, h->stream) != hipSuccess)
      r = fail(ANR_EHIP, "pq: copy failed");
  if (r == ANR_OK) r = update_pq_stats(h);
  if (r == ANR_OK) r = pq_lloyd(h, sc.res.p, sc.rn.p, n, kPqNiter);
  if (r == ANR_OK) h->pq_ready = true;
  return r;
}

}  // namespace

extern "C" {

int anr_ivf_create(int32_t dim, int32_t metric, int32_t normalize, int32_t nlist, int32_t device, anr_ivf **out) {
  if (!out) return fail(ANR_EINVAL, "out is null");
  *out = nullptr;
  if (dim <= 0 || dim > kIvfMaxDim || (dim & 1))
    return fail(ANR_EINVAL, "dim must be even and in 2..%d (got %d)", kIvfMaxDim, dim);
  if (metric != ANR_METRIC_IP && metric != ANR_METRIC_L2) return fail(ANR_EINVAL, "unknown metric %d", metric);
  if (nlist <= 0 || nlist > kIvfMaxNlist) return fail(ANR_EINVAL, "nlist must be in 1..%d (got %d)", kIvfMaxNlist, nlist);
  int ndev = anr_device_count();
  if (ndev <= 0) return fail(ANR_EHIP, "no HIP device is visible");
  if (device < 0 || device >= ndev) return fail(ANR_EINVAL, "device %d out of range (0..%d)", device, ndev - 1);
  DeviceGuard g(device);
  if (!g.ok) return fail(ANR_EHIP, "hipSetDevice(%d) failed", device);
  anr_ivf *h = new anr_ivf();
  h->dim = dim;
  h->metric = metric;
  h->normalize = normalize ? 1 : 0;
  h->nlist = nlist;
  h->device = device;
  h->list_cnt.assign(nlist, 0);
  h->list_off.assign(nlist + 1, 0);
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
    delete h;
    return fail(ANR_EHIP, "hipStreamCreate failed");
  }
  int r = alloc_centroids(h);
  if (r != ANR_OK) {
    anr_ivf_destroy(h);
    return r;
  }
  *out = h;
  return ANR_OK;
}

int anr_ivf_destroy(anr_ivf *h) {
  if (!h) return ANR_OK;
  DeviceGuard g(h->device);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;  // frees every buffer of the handle, still under the guard
  return ANR_OK;
}

int anr_ivf_train(anr_ivf *h, const float *x_host, int64_t n, int32_t niter, int64_t seed) {
  if (!h || !x_host || n < 0 || niter < 0) return fail(ANR_EINVAL, "bad argument");
  if (n < h->nlist) return fail(ANR_EINVAL, "anr_ivf_train: %lld rows cannot seed %d lists", (long long)n, h->nlist);
  if (h->pq && n < 256) return fail(ANR_EINVAL, "anr_ivf_train: %lld rows cannot train 256 PQ codes", (long long)n);
  std::lock_guard<std::mutex> lk(h->mu);
  DeviceGuard g(h->device);
  if (!g.ok) return fail(ANR_EHIP, "hipSetDevice(%d) failed", h->device);
  // subsample (at most 256 rows per list) and initial centroids: a seeded partial Fisher-Yates shuffle of the row numbers
  const int64_t m = std::min<int64_t>(n, (int64_t)256 * h->nlist);
  // PQ: its training rows are the first min(n, 256 * 256) of the same permutation
  const int64_t mpq = h->pq ? std::min<int64_t>(n, (int64_t)256 * 256) : 0;
  std::vector<int64_t> perm(n);
  std::iota(perm.begin(), perm.end(), 0);
  uint64_t st = (uint64_t)seed;
  for (int64_t i = 0; i < std::max(m, mpq); ++i) {
    const int64_t j = i + (int64_t)(splitmix(st) % (uint64_t)(n - i));
    std::swap(perm[i], perm[j]);
  }
  std::vector<int64_t> init(perm.begin(), perm.begin() + h->nlist);  // distinct rows
  std::vector<int64_t> sample(perm.begin(), perm.begin() + m);
  std::sort(sample.begin(), sample.end());
  const int dim = h->dim;
  std::vector<float> xt((size_t)m * dim), c0((size_t)h->nlist * dim);
  for (int64_t i = 0; i < m; ++i) std::memcpy(&xt[i * dim], x_host + sample[i] * dim, (size_t)dim * 4);
  for (int l = 0; l < h->nlist; ++l) std::memcpy(&c0[(size_t)l * dim], x_host + init[l] * dim, (size_t)dim * 4);
  DevBuf<float> xd, xn, cn;
  DevBuf<int32_t> asg;
  int r = need(xd, m * dim);
  if (r == ANR_OK) r = need(xn, m);
  if (r == ANR_OK) r = need(cn, h->nlist);
  if (r == ANR_OK) r = stage_rows(h, xt.data(), m, true, xd.p, xn.p);
  if (r == ANR_OK) r = stage_rows(h, c0.data(), h->nlist, true, h->cent.p, cn.p);
  if (r == ANR_OK) r = update_cstats(h);
  if (r == ANR_OK) r = lloyd(h, xd.p, xn.p, m, niter, asg);
  if (r == ANR_OK) h->trained = true;
  if (r == ANR_OK && h->pq) {
    xd.release();
    xn.release();
    std::vector<int64_t> rows(perm.begin(), perm.begin() + mpq);
    std::sort(rows.begin(), rows.end());
    r = train_pq(h, x_host, rows);
  }
  if (r == ANR_OK) r = reassign_all(h);
  if (r == ANR_OK && hipStreamSynchronize(h->stream) != hipSuccess) r = fail(ANR_EHIP, "train: stream failed");
  return r;
}

int anr_ivf_train_from_centroids(anr_ivf *h, const float *x_host, int64_t n, int32_t niter) {
  if (!h || !x_host || n <= 0 || niter < 0) return fail(ANR_EINVAL, "bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->trained) return fail(ANR_ESTATE, "anr_ivf_train_from_centroids: set the initial centroids first");
  DeviceGuard g(h->device);
  if (!g.ok) return fail(ANR_EHIP, "hipSetDevice(%d) failed", h->device);
  DevBuf<float> xd, xn;
  DevBuf<int32_t> asg;
  int r = need(xd, n * h->dim);
  if (r == ANR_OK) r = need(xn, n);
  if (r == ANR_OK) r = stage_rows(h, x_host, n, true, xd.p, xn.p);
  if (r == ANR_OK) r = lloyd(h, xd.p, xn.p, n, niter, asg);
  if (r == ANR_OK) r = reassign_all(h);
  if (r == ANR_OK && hipStreamSynchronize(h->stream) != hipSuccess) r = fail(ANR_EHIP, "train: stream failed");
  return r;
}

int anr_ivf_set_centroids(anr_ivf *h, const float *c_host) {
  if (!h || !c_host) return fail(ANR_EINVAL, "bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  DeviceGuard g(h->device);
  if (!g.ok) return fail(ANR_EHIP, "hipSetDevice(%d) failed", h->device);
  ANR_HIP(hipMemcpyAsync(h->cent.p, c_host, (size_t)h->nlist * h->dim * 4, hipMemcpyHostToDevice, h->stream));
  ANR_TRY(update_cstats(h));
  h->trained = true;
  return reassign_all(h);
}

int anr_ivf_get_centroids(anr_ivf *h, float *c_host) {
  if (!h || !c_host) return fail(ANR_EINVAL, "bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->trained) return fail(ANR_ESTATE, "the index has no centroids");
  DeviceGuard g(h->device);
  ANR_HIP(hipMemcpyAsync(c_host, h->cent.p, (size_t)h->nlist * h->dim * 4, hipMemcpyDeviceToHost, h->stream));
  ANR_HIP(hipStreamSynchronize(h->stream));
  return ANR_OK;
}

int anr_ivf_is_trained(const anr_ivf *h) { return h && h->trained && (!h->pq || h->pq_ready) ? 1 : 0; }

int anr_ivf_add(anr_ivf *h, const float *x_host, int64_t n) {
  if (!h || (!x_host && n) || n < 0) return fail(ANR_EINVAL, "bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  DeviceGuard g(h->device);
  if (!g.ok) return fail(ANR_EHIP, "hipSetDevice(%d) failed", h->device);
  return add_impl(h, x_host, n, true);
}

int anr_ivf_add_dev(anr_ivf *h, const float *x_dev, int64_t n) {
  if (!h || (!x_dev && n) || n < 0) return fail(ANR_EINVAL, "bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  DeviceGuard g(h->device);
  if (!g.ok) return fail(ANR_EHIP, "hipSetDevice(%d) failed", h->device);
  return add_impl(h, x_dev, n, false);
}

int anr_ivf_search(anr_ivf *h, const float *q_host, int64_t nq, int32_t k, int32_t nprobe, float *D, int64_t *I) {
  if (!h || nq < 0 || (nq && (!q_host || !D || !I))) return fail(ANR_EINVAL, "bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  DeviceGuard g(h->device);
  if (!g.ok) return fail(ANR_EHIP, "hipSetDevice(%d) failed", h->device);
  return search_impl(h, q_host, true, nq, k, nprobe, D, I);
}

int anr_ivf_search_devq(anr_ivf *h, const float *q_dev, int64_t nq, int32_t k, int32_t nprobe, float *D, int64_t *I) {
  if (!h || nq < 0 || (nq && (!q_dev || !D || !I))) return fail(ANR_EINVAL, "bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  DeviceGuard g(h->device);
  if (!g.ok) return fail(ANR_EHIP, "hipSetDevice(%d) failed", h->device);
  return search_impl(h, q_dev, false, nq, k, nprobe, D, I);
}

int anr_ivf_set_add_raw(anr_ivf *h, int32_t raw) {
  if (!h) return fail(ANR_EINVAL, "null handle");
  std::lock_guard<std::mutex> lk(h->mu);
  h->add_raw = raw ? 1 : 0;
  return ANR_OK;
}

int64_t anr_ivf_ntotal(const anr_ivf *h) { return h ? h->n_alive : 0; }

int anr_ivf_list_sizes(anr_ivf *h, int64_t *sizes) {
  if (!h || !sizes) return fail(ANR_EINVAL, "bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  DeviceGuard g(h->device);
  if (!g.ok) return fail(ANR_EHIP, "hipSetDevice(%d) failed", h->device);
  ANR_TRY(ensure_built(h));
  for (int l = 0; l < h->nlist; ++l) sizes[l] = h->list_cnt[l];
  return ANR_OK;
}

int anr_ivf_set_spherical(anr_ivf *h, int32_t on) {
  if (!h) return fail(ANR_EINVAL, "null handle");
  std::lock_guard<std::mutex> lk(h->mu);
  h->spherical = on ? 1 : 0;
  return ANR_OK;
}

int anr_ivf_assignments(anr_ivf *h, const int64_t *ids, int64_t n, int32_t *lists) {
  if (!h || n < 0 || (n && (!ids || !lists))) return fail(ANR_EINVAL, "bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  DeviceGuard g(h->device);
  if (!g.ok) return fail(ANR_EHIP, "hipSetDevice(%d) failed", h->device);
  for (int64_t i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= h->n_all || !h->alive[ids[i]])
      return fail(ANR_EINVAL, "anr_ivf_assignments: id %lld is not in the index", (long long)ids[i]);
  if (n == 0) return ANR_OK;
  if (h->pq) {
    for (int64_t i = 0; i < n; ++i) lists[i] = h->assign_h[ids[i]];
    return ANR_OK;
  }
  std::vector<int32_t> all(h->n_all);
  ANR_HIP(hipMemcpyAsync(all.data(), h->assign.p, (size_t)h->n_all * 4, hipMemcpyDeviceToHost, h->stream));
  ANR_HIP(hipStreamSynchronize(h->stream));
  for (int64_t i = 0; i < n; ++i) lists[i] = all[ids[i]];
  return ANR_OK;
}

int anr_ivf_last_search_stats(anr_ivf *h, int64_t *n_queries, int64_t *n_exact_rescan) {
  if (!h) return fail(ANR_EINVAL, "null handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (n_queries) *n_queries = h->last_nq;
  if (n_exact_rescan) *n_exact_rescan = h->last_exhaust;
  return ANR_OK;
}

int anr_ivf_reconstruct(anr_ivf *h, const int64_t *ids, int64_t n, float *out_host) {
  if (!h || n < 0 || (n && (!ids || !out_host))) return fail(ANR_EINVAL, "bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  DeviceGuard g(h->device);
  for (int64_t i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= h->n_all || !h->alive[ids[i]])
      return fail(ANR_EINVAL, "anr_ivf_reconstruct: id %lld is not in the index", (long long)ids[i]);
  if (n == 0) return ANR_OK;
  if (h->pq) {  // the rows live on the host
    for (int64_t i = 0; i < n; ++i)
      std::memcpy(out_host + i * h->dim, h->xh.data() + ids[i] * h->dim, (size_t)h->dim * 4);
    return ANR_OK;
  }
  ANR_TRY(need(h->rid, n));
  ANR_TRY(need(h->rout, n * h->dim));
  ANR_HIP(hipMemcpyAsync(h->rid.p, ids, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_ivf_rows, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, h->stream, h->xall.p, h->dim, h->rid.p, n,
                     h->rout.p);
  ANR_HIP(hipGetLastError());
  ANR_HIP(hipMemcpyAsync(out_host, h->rout.p, (size_t)n * h->dim * 4, hipMemcpyDeviceToHost, h->stream));
  ANR_HIP(hipStreamSynchronize(h->stream));
  return ANR_OK;
}

int anr_ivf_remove(anr_ivf *h, const int64_t *ids, int64_t n, int64_t *n_removed) {
  if (!h || n < 0 || (n && !ids)) return fail(ANR_EINVAL, "bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  DeviceGuard g(h->device);
  if (!g.ok) return fail(ANR_EHIP, "hipSetDevice(%d) failed", h->device);
  int64_t c = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t id = ids[i];
    if (id < 0 || id >= h->n_all || !h->alive[id]) continue;
    h->alive[id] = 0;
    ++c;
  }
  if (n_removed) *n_removed = c;
  if (c == 0) return ANR_OK;
  h->n_alive -= c;
  h->dirty = true;
  if (h->pq) return ANR_OK;  // the alive flags go to the device with the next rebuild
  ANR_HIP(hipMemcpyAsync(h->alive_d.p, h->alive.data(), (size_t)h->n_all, hipMemcpyHostToDevice, h->stream));
  ANR_HIP(hipStreamSynchronize(h->stream));
  return ANR_OK;
}

int anr_ivf_create_pq(int32_t dim, int32_t metric, int32_t normalize, int32_t nlist, int32_t m, int32_t nbits,
                      int32_t device, anr_ivf **out) {
  if (!out) return fail(ANR_EINVAL, "out is null");
  *out = nullptr;
  if (nbits != 8) return fail(ANR_EINVAL, "nbits must be 8 (got %d)", nbits);
  if (m <= 0 || m > kPqMaxM) return fail(ANR_EINVAL, "m must be in 1..%d (got %d)", kPqMaxM, m);
  if (dim <= 0 || dim % m != 0 || ((dim / m) & 1))
    return fail(ANR_EINVAL, "dim %d must split into m = %d sub-spaces of an even size", dim, m);
  anr_ivf *h = nullptr;
  ANR_TRY(anr_ivf_create(dim, metric, normalize, nlist, device, &h));
  DeviceGuard g(device);
  h->pq = true;
  h->m = m;
  h->m4 = (m + 3) / 4;
  h->dsub = dim / m;
  int r = need(h->cb, (int64_t)m * 256 * h->dsub);
  if (r == ANR_OK) r = need(h->cbn2, (int64_t)m * 256);
  if (r == ANR_OK) r = need(h->cbnrm, (int64_t)m * 256);
  if (r == ANR_OK) r = need(h->cbmax, m);
  if (r != ANR_OK) {
    anr_ivf_destroy(h);
    return r;
  }
  *out = h;
  return ANR_OK;
}

int anr_ivf_get_codebooks(anr_ivf *h, float *cb_host) {
  if (!h || !cb_host) return fail(ANR_EINVAL, "bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->pq) return fail(ANR_EINVAL, "not an IVF-PQ handle");
  if (!h->pq_ready) return fail(ANR_ESTATE, "the index has no codebooks");
  DeviceGuard g(h->device);
  ANR_HIP(hipMemcpyAsync(cb_host, h->cb.p, (size_t)h->m * 256 * h->dsub * 4, hipMemcpyDeviceToHost, h->stream));
  ANR_HIP(hipStreamSynchronize(h->stream));
  return ANR_OK;
}

int anr_ivf_set_codebooks(anr_ivf *h, const float *cb_host) {
  if (!h || !cb_host) return fail(ANR_EINVAL, "bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->pq) return fail(ANR_EINVAL, "not an IVF-PQ handle");
  DeviceGuard g(h->device);
  if (!g.ok) return fail(ANR_EHIP, "hipSetDevice(%d) failed", h->device);
  ANR_HIP(hipMemcpyAsync(h->cb.p, cb_host, (size_t)h->m * 256 * h->dsub * 4, hipMemcpyHostToDevice, h->stream));
  ANR_TRY(update_pq_stats(h));
  h->pq_ready = true;
  if (!h->trained) return ANR_OK;
  return reencode_all(h);
}

int anr_ivf_pq_train_from_codebooks(anr_ivf *h, const float *x_host, int64_t n, int32_t niter) {
  if (!h || !x_host || n <= 0 || niter < 0) return fail(ANR_EINVAL, "bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->pq) return fail(ANR_EINVAL, "not an IVF-PQ handle");
  if (!h->trained || !h->pq_ready)
    return fail(ANR_ESTATE, "anr_ivf_pq_train_from_codebooks: set the centroids and the initial codebooks first");
  DeviceGuard g(h->device);
  if (!g.ok) return fail(ANR_EHIP, "hipSetDevice(%d) failed", h->device);
  PqScratch sc;
  int r = need(sc.x, n * h->dim);
  if (r == ANR_OK) r = need(sc.xn, n);
  if (r == ANR_OK) r = need(sc.asg, n);
  if (r == ANR_OK) r = stage_rows(h, x_host, n, true, sc.x.p, sc.xn.p);
  if (r == ANR_OK) r = pq_residuals(h, sc.x.p, sc.xn.p, n, sc.asg.p, sc);
  if (r == ANR_OK) r = pq_lloyd(h, sc.res.p, sc.rn.p, n, niter);
  sc = PqScratch{};  // released before every row is encoded again
  if (r == ANR_OK) r = reencode_all(h);
  return r;
}

int anr_ivf_codes(anr_ivf *h, const int64_t *ids, int64_t n, int32_t *lists_out, uint8_t *codes_out) {
  if (!h || n < 0 || (n && (!ids || !lists_out || !codes_out))) return fail(ANR_EINVAL, "bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->pq) return fail(ANR_EINVAL, "not an IVF-PQ handle");
  for (int64_t i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= h->n_all || !h->alive[ids[i]])
      return fail(ANR_EINVAL, "anr_ivf_codes: id %lld is not in the index", (long long)ids[i]);
  for (int64_t i = 0; i < n; ++i) {
    lists_out[i] = h->assign_h[ids[i]];
    std::memcpy(codes_out + i * h->m, h->codes_h.data() + ids[i] * h->m, (size_t)h->m);
  }
  return ANR_OK;
}

int anr_ivf_decode(anr_ivf *h, const int64_t *ids, int64_t n, float *out_host) {
  if (!h || n < 0 || (n && (!ids || !out_host))) return fail(ANR_EINVAL, "bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->pq) return fail(ANR_EINVAL, "not an IVF-PQ handle");
  for (int64_t i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= h->n_all || !h->alive[ids[i]])
      return fail(ANR_EINVAL, "anr_ivf_decode: id %lld is not in the index", (long long)ids[i]);
  if (n == 0) return ANR_OK;
  DeviceGuard g(h->device);
  const int dim = h->dim, ds = h->dsub;
  std::vector<float> cent((size_t)h->nlist * dim), cb((size_t)h->m * 256 * ds);
  ANR_HIP(hipMemcpyAsync(cent.data(), h->cent.p, cent.size() * 4, hipMemcpyDeviceToHost, h->stream));
  ANR_HIP(hipMemcpyAsync(cb.data(), h->cb.p, cb.size() * 4, hipMemcpyDeviceToHost, h->stream));
  ANR_HIP(hipStreamSynchronize(h->stream));
  for (int64_t i = 0; i < n; ++i) {  // c_list + the codebook entries, in float32
    const float *c = cent.data() + (int64_t)h->assign_h[ids[i]] * dim;
    const uint8_t *code = h->codes_h.data() + ids[i] * h->m;
    for (int j = 0; j < h->m; ++j)
      for (int d = 0; d < ds; ++d)
        out_host[i * dim + j * ds + d] = c[j * ds + d] + cb[((size_t)j * 256 + code[j]) * ds + d];
  }
  return ANR_OK;
}

int anr_ivf_memory(anr_ivf *h, int64_t *device_bytes, int64_t *host_bytes) {
  if (!h) return fail(ANR_EINVAL, "null handle");
  std::lock_guard<std::mutex> lk(h->mu);
  DeviceGuard g(h->device);
  if (!g.ok) return fail(ANR_EHIP, "hipSetDevice(%d) failed", h->device);
  ANR_TRY(ensure_built(h));
  int64_t dev = (h->cent.cap + h->cn2.cap + h->cnrm.cap) * 4 + h->ids.cap * 8;
  int64_t host = (int64_t)h->alive.capacity() + (int64_t)(h->list_cnt.capacity() + h->list_off.capacity()) * 8;
  if (h->pq) {
    dev += (h->cb.cap + h->cbn2.cap + h->cbnrm.cap + h->cbmax.cap) * 4 + h->lcodes.cap * 4;
    host += (int64_t)h->xh.capacity() * 4 + (int64_t)h->assign_h.capacity() * 4 + (int64_t)h->codes_h.capacity();
  } else {
    dev += (h->xall.cap + h->xnrm.cap + h->assign.cap + h->xs.cap) * 4 + h->alive_d.cap + h->x16.cap * 2 + h->n2.cap * 8;
  }
  if (device_bytes) *device_bytes = dev;
  if (host_bytes) *host_bytes = host;
  return ANR_OK;
}

}  // extern "C"
