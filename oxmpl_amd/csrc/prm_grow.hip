// prm_grow.hip -- the two kernels of oxhip_prm_grow_roadmap that construction does not already have,
// on gfx950 (wave64).  Growing a roadmap continues the reference's loop (prm.rs:117-147) on the roadmap as it stands: the
// sampler, the pair search, the k-nearest selection, the edge check, the key sort and the CSR extraction are construction's
// own (prm_kernels.hip, prm_so3.hip), the liveness mask is the re-check's (prm_revalidate.hip).  What is new:
//   prm_grow_keys_kernel     one thread per CSR entry: the directed key (row << shift) | neighbour, the row found by binary
//                            search over the offsets.  The key list a grow appends to is always rebuilt this way, under the
//                            capacity the call ends with: a planted or re-checked roadmap has no current key list, and the
//                            shift changes with the capacity.
//   prm_grow_filter_kernel   one thread per candidate (j, i < j): the pair stays unless i is an old milestone that is not
//                            valid now.  Wave-ballot compaction, one atomic per wave; the order of arrival is free because the
//                            keys are sorted afterwards.  The layout is the candidates' own, whichever space found them.
// Neither kernel uses LDS or scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "oxhip_internal.hpp"
#include "rrt_device.hpp"
#include "prm_csr.hpp"

namespace oxhip {

__global__ __launch_bounds__(256) void prm_grow_keys_kernel(const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ nbrs, uint32_t n,
                                                             uint32_t n_entries, uint32_t shift, uint64_t* __restrict__ keys) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_entries) return;
    keys[t] = ((uint64_t)row_of(offsets, n, (uint32_t)t) << shift) | nbrs[t];
}

// valid[] covers the old milestones [0, n_old); a milestone of this call (i >= n_old) was valid when it was drawn.
// out holds n_cand entries, so every slot is in range; *count starts at 0 (host memset).
__global__ __launch_bounds__(256) void prm_grow_filter_kernel(const uint2* __restrict__ cand, uint32_t n_cand, const uint8_t* __restrict__ valid,
                                                               uint32_t n_old, uint2* __restrict__ out, uint32_t* count) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    bool keep = false;
    uint2 pr = make_uint2(0u, 0u);
    if (c < n_cand) {
        pr = cand[c];
        keep = pr.y >= n_old || valid[pr.y] != 0;
    }
    const uint64_t bal = __ballot(keep);
    if (bal == 0) return;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(count, (uint32_t)__popcll(bal));
    base = uni(base);
    if (keep) out[base + (uint32_t)__popcll(bal & below_mask(lane))] = pr;
}

void launch_prm_grow_keys(const uint32_t* offsets, const uint32_t* nbrs, uint32_t n, uint32_t n_entries, uint32_t shift, uint64_t* keys,
                          hipStream_t s) {
    if (n_entries == 0) return;
    hipLaunchKernelGGL(prm_grow_keys_kernel, dim3((uint32_t)(((uint64_t)n_entries + 255) / 256)), dim3(256), 0, s, offsets, nbrs, n, n_entries,
                       shift, keys);
}

void launch_prm_grow_filter(const uint2* cand, uint32_t n_cand, const uint8_t* valid, uint32_t n_old, uint2* out, uint32_t* count,
                            hipStream_t s) {
    if (n_cand == 0) return;
    hipLaunchKernelGGL(prm_grow_filter_kernel, dim3((uint32_t)(((uint64_t)n_cand + 255) / 256)), dim3(256), 0, s, cand, n_cand, valid, n_old, out,
                       count);
}

}  // namespace oxhip
