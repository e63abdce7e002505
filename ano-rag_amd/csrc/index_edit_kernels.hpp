// Kernels of the in-place edits of the flat index (anr_index_remove / anr_index_update): the stable
// compaction of the row-major arrays and the pass that re-derives the scan images and the certificate statistics from x32.
// Included by index.hip after index_kernels.hpp, whose per-value code (f16_to_12, x12_pack, x8_group) it shares with k_add.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "index_kernels.hpp"

namespace anr {

// ------------------------------------------------------------------------------------------------
// Stable compaction.  gone[0..m) are the removed rows, ascending and distinct; gm[i] = gone[i] - i is non-decreasing.
// Destination row j takes source row j + c(j), c(j) = #{i : gm[i] <= j}: the i-th removed row sits in front of survivor j
// exactly when gone[i] - i <= j (gone[i] minus the i removed rows before it is where gone[i] would land; a survivor landing
// on j comes after it).  An upper bound over gm, no prefix sums.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t edit_shift(const int64_t *gm, int64_t m, int64_t j) {
  int64_t lo = 0, hi = m;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (gm[mid] <= j) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

struct GatherParams {
  const float *src;   // [..][width] the array being compacted
  float *dst;         // the staging buffer (dst_row0 = 0) or the array itself (dst_row0 = j0)
  const int64_t *gm;  // [m]
  int64_t m;
  int64_t j0, nrows;  // destination rows [j0, j0 + nrows) of the compacted numbering
  int64_t dst_row0;
  int width;          // floats per row (dim for x32, 1 for rowbias)
};

// dst row dst_row0 + t <- src row (j0 + t) + c(j0 + t).  VEC: width is a multiple of 4 and both bases are 16-byte aligned,
// so a row is width / 4 float4s; consecutive lanes take consecutive float4s of a row.  The caller guarantees that no source
// row of the launch lies inside its destination range (the staging buffer, or a shift of at least nrows).
template <bool VEC>
__global__ __launch_bounds__(256) void k_gather_rows(GatherParams p) {
  const int upr = VEC ? p.width / 4 : p.width;  // units per row
  const int64_t total = p.nrows * upr;
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < total; u += (int64_t)gridDim.x * 256) {
    const int64_t t = u / upr;
    const int c = (int)(u - t * upr);
    const int64_t j = p.j0 + t;
    const int64_t s = j + edit_shift(p.gm, p.m, j);
    if (VEC) {
      reinterpret_cast<float4 *>(p.dst + (p.dst_row0 + t) * p.width)[c] =
          reinterpret_cast<const float4 *>(p.src + s * p.width)[c];
    } else {
      p.dst[(p.dst_row0 + t) * p.width + c] = p.src[s * p.width + c];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Re-image: k_add's arithmetic on rows that are already stored.  One block (256 threads) per 32-row tile, x32 read in place
// (no normalisation, no x32 write, rowbias of live rows untouched).  Every tile recounts its rows' statistics; tiles from
// `write_tile0` on also rewrite x16 and, where they exist, x12 / x8.  Rows at or past n_rows (the ragged tile, and the
// tiles between the new and the old extent) are written as zero bytes in every image and in rowbias: the state the
// zero-filled allocations and anr_index_reset establish, which k_add relies on for the rows it does not touch.
// ------------------------------------------------------------------------------------------------
struct ReimageParams {
  const float *x32;
  int64_t n_rows;       // rows stored after the edit
  int64_t write_tile0;  // first tile whose images are rewritten (INT64_MAX: statistics only)
  int dim, dimp, kb;
  _Float16 *x16;
  float *rowbias;       // L2 metric, or nullptr
  unsigned *stat;       // as AddParams::stat; zeroed by the caller before the pass
  unsigned *x12;
  unsigned char *x8;
};

__global__ __launch_bounds__(256) void k_reimage(ReimageParams p) {
  __shared__ float s_err[kTileRows];
  __shared__ float s_err12[kTileRows];
  __shared__ float s_err8[kTileRows];
  __shared__ float s_n2[kTileRows];
  __shared__ float s_x[kTileRows][132];

  const int tid = threadIdx.x;
  const int64_t tile = blockIdx.x;
  const int64_t trow0 = tile * kTileRows;
  const bool write = tile >= p.write_tile0;

  if (tid < kTileRows) {
    s_err[tid] = 0.0f;
    s_err12[tid] = 0.0f;
    s_err8[tid] = 0.0f;
    s_n2[tid] = 0.0f;
  }
  __syncthreads();

  for (int k0 = 0; k0 < p.dimp; k0 += 128) {
    // stage 32 x 128 stored floats through LDS
    for (int i = tid; i < kTileRows * 128; i += 256) {
      const int r = i >> 7, c = i & 127;
      const int64_t grow = trow0 + r;
      const int k = k0 + c;
      float v = 0.0f;
      if (grow < p.n_rows && k < p.dim) v = p.x32[grow * p.dim + k];
      s_x[r][c] = v;
    }
    __syncthreads();
    // 8 k-blocks x 64 lanes x 16 B (the per-value code of k_add)
    for (int i = tid; i < 8 * 64; i += 256) {
      const int kbl = i >> 6, l = i & 63;
      const int r = l & 31, h = l >> 5;
      const bool live = trow0 + r < p.n_rows;
      if (!live && !write) continue;
      half8 hv;
      unsigned r12[8];
      float e2 = 0.0f, n2 = 0.0f, e12 = 0.0f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float v = s_x[r][kbl * 16 + h * 8 + j];
        _Float16 q = (_Float16)v;
        hv[j] = q;
        float d = (float)q - v;
        if (fabsf(v) > 65504.0f) atomicOr(&p.stat[2], 1u);
        e2 += d * d;
        n2 += v * v;
        r12[j] = f16_to_12(q);
        const float d12 = (float)f12_value(r12[j]) - v;
        e12 += d12 * d12;
      }
      const int64_t blk = tile * p.kb + (k0 >> 4) + kbl;
      if (write) *reinterpret_cast<half8 *>(p.x16 + (blk * 64 + l) * 8) = hv;  // (all zero for a row past n_rows)
      if (p.x12) {
        if (write) {
          const X12 pk = x12_pack(r12);
          unsigned *o = p.x12 + (blk * 64 + l) * 3;
          o[0] = pk.h0;
          o[1] = pk.h1;
          o[2] = pk.nib;
        }
        if (live) atomicAdd(&s_err12[r], e12);
      }
      if (live) {
        atomicAdd(&s_err[r], e2);
        atomicAdd(&s_n2[r], n2);
      }
    }
    if (p.x8) {
      // one thread per (row, 32-dim group) of the stage
      for (int i = tid; i < kTileRows * 4; i += 256) {
        const int r = i & 31, g = i >> 5;
        const bool live = trow0 + r < p.n_rows;
        if (!live && !write) continue;
        unsigned short sb = 0;
        uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;  // a row past n_rows: zero bytes, not the code of 0.0
        if (live) atomicAdd(&s_err8[r], x8_group(&s_x[r][g * 32], 1, &sb, &lo, &hi));
        if (write) {
          const int m = (k0 >> 5) + g;
          unsigned char *t = p.x8 + tile * p.kb * kX8TileBytesPerKb;
          *reinterpret_cast<uint4 *>(t + x8_pair(m) + r * 16) = lo;
          *reinterpret_cast<uint4 *>(t + x8_pair(m) + (r + 32) * 16) = hi;
          *reinterpret_cast<unsigned short *>(t + x8_scale_at(m, r)) = sb;
        }
      }
    }
    __syncthreads();
  }
  if (tid < kTileRows) {
    const int64_t grow = trow0 + tid;
    if (grow < p.n_rows) {
      // 1.0001: slack for the f32 accumulation of the partial sums above
      atomicMax(&p.stat[0], __float_as_uint(sqrtf(s_n2[tid]) * 1.0001f));
      atomicMax(&p.stat[1], __float_as_uint(sqrtf(s_err[tid]) * 1.0001f));
      if (p.x12) atomicMax(&p.stat[3], __float_as_uint(sqrtf(s_err12[tid]) * 1.0001f));
      if (p.x8) atomicMax(&p.stat[4], __float_as_uint(sqrtf(s_err8[tid]) * 1.0001f));
    } else if (write && p.rowbias) {
      p.rowbias[grow] = 0.0f;
    }
  }
}

}  // namespace anr
