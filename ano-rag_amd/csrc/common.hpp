// Shared host-side helpers for libanorag_hip.so: error reporting and HIP call checking, the device guard, and the one
// owner of device memory outside the scan and the encoder — DevBuf (a typed, move-only device buffer with a capacity),
// ArenaLayout (offsets of the arrays carved from one buffer) and Events (HIP-event timing of a call).  The f64 MFMA Gram
// tile that diversity.hip and cluster_quality.hip share is in gram_f64.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "anorag.h"

namespace anr {

// thread-local last-error text behind anr_last_error()
std::string &last_error_ref();
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define ANR_HIP(expr)                                                                            \
  do {                                                                                           \
    hipError_t _e = (expr);                                                                      \
    if (_e != hipSuccess)                                                                        \
      return anr::fail(ANR_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                       __LINE__);                                                                \
  } while (0)

#define ANR_TRY(expr)       \
  do {                      \
    int _r = (expr);        \
    if (_r != ANR_OK) return _r; \
  } while (0)

static inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
static inline int64_t ceil_div(int64_t x, int64_t m) { return (x + m - 1) / m; }

// RAII device guard: every entry point switches to the handle's device and restores the caller's.
struct DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) ok = (hipSetDevice(dev) == hipSuccess);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// A typed device buffer with its capacity in elements.  Move-only; frees in its destructor, so a buffer of one call is
// declared after the DeviceGuard it must not outlive, and a member of a handle is freed where the handle is deleted.
template <typename T>
struct DevBuf {
  T *p = nullptr;
  int64_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      release();
      p = o.p, cap = o.cap;
      o.p = nullptr, o.cap = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  // Room for n elements.  Nothing happens if it is there; otherwise the old block is freed (its contents are not kept)
  // and max(n, want, 1) elements are allocated: `want` is the caller's growth rule, and a buffer of no elements still has
  // a pointer.  `what` names the caller in the error text, `purpose` the buffer where the caller has several.
  int alloc(int64_t n, const char *what, int64_t want = 0, const char *purpose = nullptr) {
    if (p && n <= cap) return ANR_OK;
    release();
    const int64_t nc = std::max<int64_t>(std::max(n, want), 1);
    const size_t bytes = (size_t)nc * sizeof(T);
    if (hipMalloc(reinterpret_cast<void **>(&p), bytes) != hipSuccess) {
      p = nullptr;
      (void)hipGetLastError();  // the error is sticky
      return fail(ANR_EHIP, "%s: could not allocate %zu bytes of device memory%s%s", what, bytes, purpose ? " for " : "",
                  purpose ? purpose : "");
    }
    cap = nc;
    return ANR_OK;
  }
};

// byte offsets of the arrays of one call inside one device buffer, every one aligned to ALIGN bytes
template <size_t ALIGN>
struct ArenaLayout {
  size_t at = 0;  // the end of what was taken so far
  size_t take(size_t bytes) {
    const size_t r = at;
    at = (at + bytes + ALIGN - 1) & ~(ALIGN - 1);
    return r;
  }
};

// N HIP events for the developer timing of one call: nothing is created or recorded until init()
template <int N>
struct Events {
  hipEvent_t e[N] = {};
  bool on = false;
  int init() {
    on = true;
    for (auto &x : e) ANR_HIP(hipEventCreate(&x));
    return ANR_OK;
  }
  int mark(int i, hipStream_t st) {
    if (on) ANR_HIP(hipEventRecord(e[i], st));
    return ANR_OK;
  }
  int elapsed(int i, int j, float *ms) {
    ANR_HIP(hipEventElapsedTime(ms, e[i], e[j]));
    return ANR_OK;
  }
  ~Events() {
    for (auto &x : e)
      if (x) (void)hipEventDestroy(x);
  }
};

int device_cu_count(int device);

// device-wide stable radix sort of (key, u32 value) pairs (radix_sort.hip); temp: radix_sort_temp_bytes(n) bytes of device
// memory; equal keys keep their input order, also when descending
size_t radix_sort_temp_bytes(int64_t n);
int radix_sort_pairs_u64(void *temp, const unsigned long long *k_in, unsigned long long *k_out, const unsigned *v_in,
                         unsigned *v_out, int64_t n, bool descending, hipStream_t st);
int radix_sort_pairs_f32(void *temp, const float *k_in, float *k_out, const unsigned *v_in, unsigned *v_out, int64_t n,
                         bool descending, hipStream_t st);

// top-k beyond the select window (largek.hip): full device sort of one query's exact scores
struct LargeKScratch {
  DevBuf<unsigned> iota, rows;
  DevBuf<float> keys;
  DevBuf<unsigned char> temp;
  int64_t n = 0;
};
int sort_topk(const float *scores_dev, int64_t n, int k, bool larger_is_better, int64_t id_offset, float *D_row,
              int64_t *I_row, LargeKScratch *s, hipStream_t st);
void free_largek(LargeKScratch *s);

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel, current device): the attribute belongs to the
// device's copy of the kernel, so a process that drives several GPUs needs it on each; thread-safe
int ensure_dynamic_lds(const void *kernel, int bytes);

// XCD-aware workgroup -> tile mapping for GEMM-shaped grids (MB x NB tiles).  Workgroups are dealt round-robin
// over the 8 XCDs (b and b + 8 share one; observed, speed only), each XCD has its own L2, and the 32 workgroups
// an XCD runs at a time walk K in step — so the 32 are given a P x Q patch of tiles (P * Q = 32): the P + Q
// operand blocks of the patch are fetched from outside the XCD once and re-used from its L2 by the others,
// instead of every workgroup streaming both of its operands from the Infinity Cache / HBM (measured: the
// 256 x 256 self-join tile at K = 768 was pinned at ~6.5 TB/s of L2 misses = 840 TFLOP/s).
struct PatchGrid {
  int MB, NB, P, Q;
  int patches_n;      // patches along N
  int64_t n_patches;
  int contig;         // 1: XCD x takes the CONSECUTIVE patches [x * per_xcd, (x + 1) * per_xcd) — with patches numbered
                      // N-fastest an XCD then keeps the same M panels in its L2 while it walks the N panels (GEMM: every
                      // activation panel is fetched by ONE XCD only); 0: patches dealt round-robin over the XCDs
  // workgroups to launch: whole patches, a multiple of 8 of them
  __host__ __device__ int64_t per_xcd() const { return (n_patches + 7) / 8; }
  __host__ __device__ int64_t grid() const { return per_xcd() * 8 * (int64_t)(P * Q); }
};

static inline PatchGrid make_patch_grid(int64_t MB, int64_t NB) {
  // the 32-tile patch shape that wastes the fewest slots, squarer first
  static const int shapes[6][2] = {{4, 8}, {8, 4}, {2, 16}, {16, 2}, {1, 32}, {32, 1}};
  PatchGrid best{};
  int64_t best_slots = -1;
  for (const auto &sh : shapes) {
    const int64_t pm = ceil_div(MB, sh[0]), pn = ceil_div(NB, sh[1]);
    const int64_t slots = (pm * pn + 7) / 8 * 8 * 32;
    if (best_slots < 0 || slots < best_slots) {
      best_slots = slots;
      best = PatchGrid{(int)MB, (int)NB, sh[0], sh[1], (int)pn, pm * pn, 0};
    }
  }
  return best;
}

#if defined(__HIPCC__)
// false: this workgroup has no tile (grid padding)
__device__ __forceinline__ bool patch_tile(const PatchGrid &g, int64_t wg, int &bm, int &bn) {
  const int xcd = (int)(wg & 7);
  const int64_t local = wg >> 3;
  const int within = (int)(local % (g.P * g.Q));
  const int64_t patch = g.contig ? xcd * g.per_xcd() + local / (g.P * g.Q) : (local / (g.P * g.Q)) * 8 + xcd;
  if (patch >= g.n_patches) return false;
  bm = (int)(patch / g.patches_n) * g.P + within / g.Q;
  bn = (int)(patch % g.patches_n) * g.Q + within % g.Q;
  return bm < g.MB && bn < g.NB;
}
#endif

}  // namespace anr
