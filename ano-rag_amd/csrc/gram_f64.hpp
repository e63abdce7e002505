// The float64 Gram tile of the analytics kernels: raw products G = A B^T of stored float32 rows with
// v_mfma_f64_16x16x4_f64 (diversity.hip, cluster_quality.hip; kmeans.hip keeps its own loops over the same lane map).
//
// Lane map.  Operand lanes: A[i][k] and B[k][j] both sit in lane (i or j) + 16 k, one double each, i, j < 16, k < 4.
// Result register r of a lane is row (lane >> 4) + 4 r, column lane & 15 of the 16 x 16 block.
//
// Determinism rule.  Every tile, whatever its position, runs the same ceil(dim / 64) * 16 MFMA steps over k in ascending
// order, with padding rows and k beyond dim as exact zeros.  A product of two float32 values is exact in float64, so G_ij
// is one fixed sequence of additions of exact products of rows i and j — the same one on the diagonal, so identical rows
// have G_ii = G_ij = G_jj bit for bit, and every kernel that instantiates this tile reads the same G.  The files that use
// it are compiled without multiply-add contraction (Makefile, EXACT).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace anr {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int kGramKC = 64;  // k-chunk staged through LDS

// One tile by a workgroup of WM x WN waves.  Wave w = WN * wi + wj owns tile rows 16 wi .. 16 wi + 15 and NB 16-column
// blocks: block b is tile columns 16 (NB wj + b) .. + 15, in acc[b].  ra / rb name the stored rows of the tile's rows and
// columns (16 WM = 16 WN NB of each, in LDS, -1 = padding); As / Bs are the staging arrays, LD floats a row.  Per
// k-chunk: stage both operands as float, then the 16 steps in ascending k.  Ends with a barrier.
template <int WM, int WN, int NB, int LD>
__device__ __forceinline__ void gram_f64_tile(const float *__restrict__ x32, int dim, const int64_t *ra, const int64_t *rb,
                                              float (*As)[LD], float (*Bs)[LD], double4_t acc[NB]) {
  constexpr int kRows = 16 * WM, kNT = 64 * WM * WN;
  constexpr int kSteps = 16 / NB;  // k-steps unrolled together: 16 MFMAs a body, whatever the block count
  static_assert(16 * WN * NB == kRows, "the tile is square");
  static_assert(LD >= kGramKC, "a row of LDS holds a k-chunk");
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wi = w / WN, wj = w % WN;
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[b] = double4_t{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < dim; k0 += kGramKC) {
    for (int e = tid; e < kRows * kGramKC; e += kNT) {
      const int r = e / kGramKC, k = e % kGramKC, kk = k0 + k;
      float va = 0.f, vb = 0.f;
      if (kk < dim) {
        if (ra[r] >= 0) va = x32[ra[r] * dim + kk];
        if (rb[r] >= 0) vb = x32[rb[r] * dim + kk];
      }
      As[r][k] = va;
      Bs[r][k] = vb;
    }
    __syncthreads();
#pragma unroll kSteps
    for (int ks = 0; ks < kGramKC; ks += 4) {
      const double a = (double)As[wi * 16 + (lane & 15)][ks + (lane >> 4)];
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const double bv = (double)Bs[(wj * NB + b) * 16 + (lane & 15)][ks + (lane >> 4)];
        acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, acc[b], 0, 0, 0);
      }
    }
    __syncthreads();
  }
}

}  // namespace anr
