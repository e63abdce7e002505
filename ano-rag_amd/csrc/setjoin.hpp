// Set-overlap join (setjoin.hip): the limits shared by the entry points and the kernels.
#pragma once
#include <cstdint>

namespace anr {

constexpr int kSjThreads = 256;          // one workgroup per row of the co-occurrence join
constexpr int kSjDefaultSlots = 4096;    // LDS table slots: 16 bytes of LDS each -> 65 KiB per workgroup, two per CU
constexpr int kSjMinSlots = 64, kSjMaxSlots = 4096;
constexpr int64_t kSjMaxRowLen = 1 << 20;  // items per row: keeps a pass's shared-id offsets inside 32 bits
constexpr int kSjPairLanes = 8;          // lanes that share one pair of anr_setjoin_pair_counts

// a pass of the table holds at most 3/4 of its slots as distinct keys
constexpr int sj_table_fill(int slots) { return slots - slots / 4; }

// the table's keys and counts, the compaction buffer (16 bytes a slot), 256 partial sums and the pass's counters
constexpr int sj_lds_bytes(int slots) { return slots * 16 + kSjThreads * 4 + 32; }

#if defined(__HIPCC__)
// the kernels of setjoin.hip that turn a CSR into postings around the one radix sort, and the one-workgroup exclusive
// scan of per-row counts (out[n] = the total); tfidf.hip launches them too
__global__ void k_sj_keys(const int64_t *indptr, const int32_t *items, int64_t n_rows, int64_t nnz, unsigned long long *keys);
__global__ void k_sj_post_ptr(const unsigned long long *sorted, int64_t nnz, int64_t n_items, int64_t *post_ptr);
__global__ void k_sj_post_rows(const unsigned long long *sorted, int64_t nnz, int32_t *post_rows);
__global__ void k_sj_scan(const int64_t *in, int64_t n, int64_t *out);
#endif

}  // namespace anr
