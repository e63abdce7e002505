// The MFMA product of one 256 x 256 block pair of the blocked f16 image (index_kernels.hpp has the layout): the tile loop
// of the self join (k_join_r, index_kernels.hpp), which the DBSCAN tile walks (cluster_kernels.hpp) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace anr {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kTileRows = 32;    // corpus rows per MFMA tile

// The operand fragments travel global -> VGPR -> LDS (ds_write_b128): two LDS slots of four k-steps; the
// fragments of stage s + 1 wait in registers while stage s is multiplied and are written into the other slot in
// the middle of it.  Variants measured on this kernel and dropped, all within 5 % of each other (820-880
// TFLOP/s at K = 768, ~42 % MFMA utilisation at the 1.9 GHz the chip holds under this load): operands through
// global_load_lds and a three-slot ring; 4 waves x (128 x 128) with double-buffered fragment reads (half the
// LDS reads per MFMA); non-persistent workgroups; linear instead of XCD-patched tile order (L2 hit rate 76 % with
// the patches).  What is left is the fill and drain of the 12-stage K loop per tile and the epilogue (~25 % of
// a tile's time at K = 768; 934 TFLOP/s at 300 k rows, 891 at K = 1024).
// The product of one 256 x 256 block pair, shared by the self join and the DBSCAN tile walks (cluster_kernels.hpp): the
// workgroup's 8 waves (4 x 2) leave x16_i . x16_j of rows i = (tb0 + 2 wm + m) * 32 + (lane & 31) and
// j = (nb0 + 4 wn + n) * 32 + 4 (lane >> 5) + (r & 3) + 8 (r >> 2) in acc[m][n][r].  lds: [2][S][F][64] uint4 (128 KiB);
// the last barrier inside leaves it free for the caller.
__device__ __forceinline__ void join_tile_mma(const uint4 *x16, int kb, int64_t n_tiles, int64_t tb0, int64_t nb0,
                                              uint4 *lds, int lane, int wave, floatx16 (&acc)[2][4]) {
  constexpr int TM = 8, TN = 8, S = 4, F = TM + TN, LPW = S * F / 8;
  const int wm = wave >> 1, wn = wave & 1;
  const u32x4 *xl = reinterpret_cast<const u32x4 *>(x16) + lane;  // native vectors: HIP's uint4 struct kept the staging array in scratch
  int64_t src[LPW];  // uniform offsets (uint4 units) of this wave's fragments at k-step 0
  int dst[LPW];
#pragma unroll
  for (int i = 0; i < LPW; ++i) {
    const int f = wave * LPW + i, ks = f / F, idx = f % F;
    int64_t tile = idx < TM ? tb0 + idx : nb0 + idx - TM;
    if (tile >= n_tiles) tile = n_tiles - 1;  // clamp: masked at emit
    src[i] = (tile * kb + ks) * 64;
    dst[i] = (ks * F + idx) * 64;
  }
  u32x4 *ldsl = reinterpret_cast<u32x4 *>(lds) + lane;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;
  const int nstages = kb / S;
  constexpr int BUF = S * F * 64;  // uint4 per slot
  u32x4 stg[LPW];
#pragma unroll
  for (int i = 0; i < LPW; ++i) stg[i] = xl[src[i]];
#pragma unroll
  for (int i = 0; i < LPW; ++i) ldsl[dst[i]] = stg[i];
  if (nstages > 1) {
#pragma unroll
    for (int i = 0; i < LPW; ++i) stg[i] = xl[src[i] + (int64_t)S * 64];
  }
  __syncthreads();
  for (int s = 0; s < nstages; ++s) {
    const uint4 *L = lds + (s & 1) * BUF + lane;
#pragma unroll
    for (int ks = 0; ks < S; ++ks) {
      half8 a[2], b[4];
#pragma unroll
      for (int m = 0; m < 2; ++m) a[m] = __builtin_bit_cast(half8, L[(ks * F + 2 * wm + m) * 64]);
#pragma unroll
      for (int n = 0; n < 4; ++n) b[n] = __builtin_bit_cast(half8, L[(ks * F + TM + 4 * wn + n) * 64]);
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(b[n], a[m], acc[m][n], 0, 0, 0);
      if (ks == 1 && s + 1 < nstages) {
        // stage s + 1 has had a k-step and a half to arrive: park it in the other slot (free since the barrier
        // that ended stage s - 1) and request stage s + 2
        __builtin_amdgcn_sched_barrier(0);
        u32x4 *W = ldsl + ((s + 1) & 1) * BUF;
#pragma unroll
        for (int i = 0; i < LPW; ++i) W[dst[i]] = stg[i];
        if (s + 2 < nstages) {
#pragma unroll
          for (int i = 0; i < LPW; ++i) stg[i] = xl[src[i] + (int64_t)(s + 2) * S * 64];
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // LDS writes of this wave done, then the workgroup barrier — NOT __syncthreads(), whose vmcnt(0) would also
    // wait for the stage s + 2 loads just requested
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  }
}

}  // namespace anr
