// prm_csr.hpp -- what the kernels that walk a roadmap's CSR share (prm_batch.hip, prm_shortest.hip, prm_revalidate.hip).
#pragma once
#include "rrt_device.hpp"

namespace oxhip {

constexpr uint32_t kRoot = 0x7FFFFFFFu;   // parent word of a start connection / a source: what prm_batch_paths_kernel never follows
                                          // (parent_map's Some(None)); milestone indices are < 2^26

// Words another wave of the workgroup wrote (plain stores and atomics alike) are read and written at L2.
__device__ __forceinline__ uint32_t ld_l2(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_l2(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the row of CSR entry e: the last u with offsets[u] <= e (rows may be empty; offsets[0] = 0 <= e < offsets[n])
__device__ __forceinline__ uint32_t row_of(const uint32_t* __restrict__ offsets, uint32_t n, uint32_t e) {
    uint32_t lo = 0, hi = n;   // the answer lies in [lo, hi)
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

// the entry of row `row` that holds `want` (rows ascending), 0xFFFFFFFF when it holds none
__device__ __forceinline__ uint32_t row_find(const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ nbrs, uint32_t row,
                                             uint32_t want) {
    uint32_t lo = offsets[row], hi = offsets[row + 1];
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (nbrs[mid] < want) lo = mid + 1; else hi = mid;
    }
    return lo < offsets[row + 1] && nbrs[lo] == want ? lo : 0xFFFFFFFFu;
}

}  // namespace oxhip
