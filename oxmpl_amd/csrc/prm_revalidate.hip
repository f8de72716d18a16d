// prm_revalidate.hip -- a roadmap planted from the host, and a roadmap re-checked against the scene as it stands now
// (oxhip_prm_set_roadmap / oxhip_prm_revalidate), on gfx950 (wave64).
//
// Planting: two kernels check the caller's CSR before it replaces the handle's -- the offsets (start at 0, never decrease), then
// per entry the neighbour's range, no self-loop, rows strictly ascending, symmetry.  Every rule has one result word that ends up
// holding the lowest offending row (atomicMin), so the refusal's message does not depend on the order of arrival.
//
// Re-checking (the semantics are this build's own; the reference has no such call):
//   1. prm_reval_valid_kernel   valid[i] = is_valid(milestone i), one thread per milestone, over SeqSpace<DIM> (seq_space.hpp)
//   2. prm_reval_emit_kernel    one thread per CSR entry (u -> v): v < u and both ends valid -> (entry, u, v) joins the pair list
//                               (one atomic per wave, from a ballot, as prm_edge_kernel appends its keys)
//   3. prm_reval_check_kernel   R^n, one thread per pair: check_motion(from = milestone u, to = milestone v), construction's own
//                               direction and device function (motion_valid_seq); a kept pair sets the keep byte of its own
//                               entry.  prm_reval_mirror_kernel then gives every upper entry (u -> v, v > u) the byte of its
//                               mirror (u in row v, by binary search).
//                               SO(3): the pair list, in construction's candidate layout, goes through construction's own
//                               prm_so3_edge_kernel; prm_reval_keys_kernel turns the keys it emits into keep bytes
//   4. exclusive scan of the keep bytes (rocPRIM, the library prm_sort_keys uses), then prm_reval_compact_kernel: the new
//      offsets, and the kept neighbours in their old order -- rows stay ascending, no key sort, no CSR rebuild.
// No kernel of this file uses LDS (construction's SO(3) edge kernel, which step 3 runs, stages its cones there).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "oxhip_internal.hpp"
#include "rrt_device.hpp"
#include "prm_csr.hpp"
#include "seq_space.hpp"

namespace oxhip {

// ------------------------------------------------------------------------------------------------
// planting: the structure rules.  viol[rule] starts at 0xFFFFFFFF and ends as the lowest offending row.

// offsets as the caller gave them (64-bit, offsets[n] <= 0xFFFFFFFF checked by the host) -> the handle's 32-bit ones
__global__ __launch_bounds__(256) void prm_plant_offsets_kernel(const uint64_t* __restrict__ off64, uint32_t n, uint32_t* __restrict__ off32,
                                                                 uint32_t* viol) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    const uint64_t a = off64[i];
    off32[i] = (uint32_t)a;
    if (i == 0 && a != 0) atomicMin(&viol[kPlantOffsetsStart], 0u);
    if (i < n && off64[i + 1] < a) atomicMin(&viol[kPlantOffsetsOrder], i);
}

// one thread per entry; runs only when the offsets passed (so every row lies inside [0, n_entries))
__global__ __launch_bounds__(256) void prm_plant_entries_kernel(const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ nbrs,
                                                                 uint32_t n, uint32_t n_entries, uint32_t* viol) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_entries) return;
    const uint32_t e = (uint32_t)t;
    const uint32_t u = row_of(offsets, n, e), v = nbrs[e];
    if (v >= n) { atomicMin(&viol[kPlantRange], u); return; }
    if (v == u) atomicMin(&viol[kPlantSelfLoop], u);
    if (e > offsets[u] && nbrs[e - 1] >= v) atomicMin(&viol[kPlantUnsorted], u);
    // (an unsorted row v can hide u from the search: the host reports the rules in this order, so that refusal comes first)
    if (row_find(offsets, nbrs, v, u) == 0xFFFFFFFFu) atomicMin(&viol[kPlantAsymmetric], u);
}

// ------------------------------------------------------------------------------------------------
// 1. milestone validity (the bits of oxhip_rrt_batch_is_valid: obstacle_hit / so3_cone_hit per obstacle)

template <int DIM>
__global__ __launch_bounds__(256) void prm_reval_valid_kernel(typename SeqSpace<DIM>::Checker p, const double* __restrict__ ms, uint32_t n,
                                                               uint8_t* __restrict__ valid, uint32_t* counters) {
    using Space = SeqSpace<DIM>;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    bool bad = false;
    if (i < n) {
        double s[Space::W];
        Space::load(ms + (size_t)i * Space::W, s);
        bad = !Space::state_valid(Space::vgpr_pointers(p), s);
        valid[i] = bad ? 0 : 1;
    }
    const uint64_t bal = __ballot(bad);
    if (bal != 0 && lane == 0) atomicAdd(&counters[kRevalInvalid], (uint32_t)__popcll(bal));
}

// ------------------------------------------------------------------------------------------------
// 2. the pairs to check: entries (u -> v) with v < u between two valid milestones.  The keep bytes start at 0 (host memset).

__global__ __launch_bounds__(256) void prm_reval_emit_kernel(const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ nbrs,
                                                              const uint8_t* __restrict__ valid, uint32_t n, uint32_t n_entries,
                                                              uint4* __restrict__ pairs, uint2* __restrict__ cand, uint32_t pair_cap,
                                                              uint32_t* counters) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    bool take = false;
    uint32_t u = 0, v = 0;
    if (t < n_entries) {
        v = nbrs[t];
        u = row_of(offsets, n, (uint32_t)t);
        take = v < u && valid[u] != 0 && valid[v] != 0;
    }
    const uint64_t bal = __ballot(take);
    if (bal == 0) return;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&counters[kRevalPairs], (uint32_t)__popcll(bal));
    base = uni(base);
    if (take) {
        const uint32_t slot = base + (uint32_t)__popcll(bal & below_mask(lane));
        if (slot < pair_cap) {   // (a symmetric CSR holds exactly n_entries / 2 such entries)
            if (cand != nullptr) cand[slot] = make_uint2(u, v);   // SO(3): construction's candidate layout (j, i < j), for its own edge kernel
            else pairs[slot] = make_uint4((uint32_t)t, u, v, 0u);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// 3. check_motion per pair (from = the higher index u, to = the lower one v: prm.rs:134, as prm_edge_kernel)

template <int DIM>
__global__ __launch_bounds__(256) void prm_reval_check_kernel(DevParams p, const double* __restrict__ ms, const uint4* __restrict__ pairs,
                                                               uint32_t n_pairs, uint8_t* __restrict__ keep) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_pairs) return;
    const uint4 pr = pairs[c];
    using Space = SeqSpace<DIM>;
    double from[DIM], to[DIM];
    Space::load(ms + (size_t)pr.y * DIM, from);
    Space::load(ms + (size_t)pr.z * DIM, to);
    // a planted milestone may lie outside the bounds: the filter's margin with this motion's ends in play (the verdict is construction's)
    const double filt = Space::motion_margin(p.filt_abs, from, to);
    if (Space::motion_valid(Space::vgpr_pointers(p), from, to, filt)) keep[pr.x] = 1;
}

// SO(3): the pairs go through construction's own prm_so3_edge_kernel (prm_so3.hip), which appends both directed keys
// (u << shift | v, v << shift | u) of every valid motion; one thread per key finds its entry (v in row u) and keeps it.
// Both directions arrive as keys, so no mirror pass is needed.
__global__ __launch_bounds__(256) void prm_reval_keys_kernel(const uint64_t* __restrict__ keys, const PrmState* __restrict__ state,
                                                              uint32_t key_cap, uint32_t shift, const uint32_t* __restrict__ offsets,
                                                              const uint32_t* __restrict__ nbrs, uint32_t n, uint8_t* __restrict__ keep) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= key_cap || k >= state->n_keys) return;   // (the count stays on the device: no read-back between the two kernels)
    const uint64_t key = keys[k];
    const uint32_t u = (uint32_t)(key >> shift), v = (uint32_t)(key & ((1ull << shift) - 1ull));
    if (u >= n) return;
    const uint32_t e = row_find(offsets, nbrs, u, v);
    if (e != 0xFFFFFFFFu) keep[e] = 1;
}

// the mirror entries: (u -> v) with v > u takes the keep byte of (v -> u), found by binary search for u in row v.  Only the
// lower entries were written above and only the upper ones are written here, so no byte has two writers.
__global__ __launch_bounds__(256) void prm_reval_mirror_kernel(const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ nbrs, uint32_t n,
                                                                uint32_t n_entries, uint8_t* keep) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_entries) return;
    const uint32_t v = nbrs[t], u = row_of(offsets, n, (uint32_t)t);
    if (v <= u) return;
    const uint32_t lower = row_find(offsets, nbrs, v, u);
    if (lower != 0xFFFFFFFFu && keep[lower] != 0) keep[t] = 1;
}

// ------------------------------------------------------------------------------------------------
// 4. compaction: pos = exclusive scan of keep.  One thread per entry moves its neighbour, one per row (and one for
// offsets[n]) rewrites its offset -- each thread reads and writes its own offset only, so the offsets change in place.

__global__ __launch_bounds__(256) void prm_reval_compact_kernel(uint32_t* offsets, const uint32_t* __restrict__ nbrs, const uint8_t* __restrict__ keep,
                                                                 const uint32_t* __restrict__ pos, uint32_t n, uint32_t n_entries,
                                                                 uint32_t* __restrict__ nbrs_out) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n_entries && keep[t]) nbrs_out[pos[t]] = nbrs[t];
    if (t <= n) {
        const uint32_t o = offsets[t];
        offsets[t] = o < n_entries ? pos[o] : pos[n_entries - 1] + keep[n_entries - 1];   // (n_entries > 0: the host handles 0)
    }
}

// ------------------------------------------------------------------------------------------------
// launchers

static uint32_t blocks_for(uint64_t work) { return (uint32_t)((work + 255) / 256); }

void launch_prm_plant_offsets(const uint64_t* off64, uint32_t n, uint32_t* off32, uint32_t* viol, hipStream_t s) {
    hipLaunchKernelGGL(prm_plant_offsets_kernel, dim3(blocks_for((uint64_t)n + 1)), dim3(256), 0, s, off64, n, off32, viol);
}

void launch_prm_plant_entries(const uint32_t* offsets, const uint32_t* nbrs, uint32_t n, uint32_t n_entries, uint32_t* viol, hipStream_t s) {
    if (n_entries == 0) return;
    hipLaunchKernelGGL(prm_plant_entries_kernel, dim3(blocks_for(n_entries)), dim3(256), 0, s, offsets, nbrs, n, n_entries, viol);
}

void launch_prm_reval_valid(bool so3, const DevParams& p, const double* ms, uint32_t n, uint8_t* valid, uint32_t* counters, hipStream_t s) {
    space_dispatch(prm_space(so3), p.dim, [&](auto d) {
        constexpr int D = decltype(d)::value;
        hipLaunchKernelGGL(prm_reval_valid_kernel<D>, dim3(blocks_for(n)), dim3(256), 0, s, SeqSpace<D>::checker(p), ms, n, valid, counters);
    });
}

void launch_prm_reval_emit(const uint32_t* offsets, const uint32_t* nbrs, const uint8_t* valid, uint32_t n, uint32_t n_entries, uint4* pairs,
                           uint2* cand, uint32_t pair_cap, uint32_t* counters, hipStream_t s) {
    if (n_entries == 0) return;
    hipLaunchKernelGGL(prm_reval_emit_kernel, dim3(blocks_for(n_entries)), dim3(256), 0, s, offsets, nbrs, valid, n, n_entries, pairs, cand,
                       pair_cap, counters);
}

void launch_prm_reval_check(const DevParams& p, const double* ms, const uint32_t* offsets, const uint32_t* nbrs, uint32_t n, uint32_t n_entries,
                            const uint4* pairs, uint32_t n_pairs, uint8_t* keep, hipStream_t s) {
    if (n_pairs == 0) return;
    dim_dispatch(p.dim, [&](auto d) {
        constexpr int D = decltype(d)::value;
        hipLaunchKernelGGL(prm_reval_check_kernel<D>, dim3(blocks_for(n_pairs)), dim3(256), 0, s, p, ms, pairs, n_pairs, keep);
    });
    hipLaunchKernelGGL(prm_reval_mirror_kernel, dim3(blocks_for(n_entries)), dim3(256), 0, s, offsets, nbrs, n, n_entries, keep);
}

void launch_prm_reval_keys(const uint64_t* keys, const PrmState* state, uint32_t key_cap, uint32_t shift, const uint32_t* offsets,
                           const uint32_t* nbrs, uint32_t n, uint8_t* keep, hipStream_t s) {
    if (key_cap == 0) return;
    hipLaunchKernelGGL(prm_reval_keys_kernel, dim3(blocks_for(key_cap)), dim3(256), 0, s, keys, state, key_cap, shift, offsets, nbrs, n, keep);
}

struct KeepToCount {
    __host__ __device__ uint32_t operator()(uint8_t k) const { return k; }
};

hipError_t prm_reval_scan(void* tmp, size_t& tmp_bytes, const uint8_t* keep, uint32_t* pos, uint32_t n_entries, hipStream_t s) {
    auto in = rocprim::make_transform_iterator(keep, KeepToCount{});
    return rocprim::exclusive_scan(tmp, tmp_bytes, in, pos, 0u, (size_t)n_entries, rocprim::plus<uint32_t>(), s);
}

void launch_prm_reval_compact(uint32_t* offsets, const uint32_t* nbrs, const uint8_t* keep, const uint32_t* pos, uint32_t n, uint32_t n_entries,
                              uint32_t* nbrs_out, hipStream_t s) {
    if (n_entries == 0) return;
    const uint64_t work = n_entries > (uint64_t)n + 1 ? n_entries : (uint64_t)n + 1;
    hipLaunchKernelGGL(prm_reval_compact_kernel, dim3(blocks_for(work)), dim3(256), 0, s, offsets, nbrs, keep, pos, n, n_entries, nbrs_out);
}

}  // namespace oxhip
