// prm_components.hip -- the connected components of a roadmap, and the roadmap pruned by a keep mask
// (oxhip_prm_components / oxhip_prm_prune), on gfx950 (wave64).  Only the CSR is read: no obstacle, no state.
//
// Components: a lock-free union-find over the CSR (ECL-CC's shape).  parent[x] <= x always holds and only a root (parent[x] == x)
// is ever linked, under a smaller index, so the root that survives is the component's lowest index whichever thread wins.
//   1. prm_cc_self_kernel      parent[v] = v, count[v] = 0; the summary words to 0
//   2. prm_cc_init_kernel      one thread per CSR entry (v, u): parent[v] = the first (live) neighbour below v.  Rows are ascending,
//                              so that is the row's minimum: within a wave the first taking lane of each row's run does the
//                              atomicMin, so a row of any length costs one atomic per wave it spans.
//   3. prm_cc_hook_kernel      one thread per CSR entry (v, u) with u < v: both roots by path halving, the larger linked under the
//                              smaller by compare-and-swap; a lost swap continues from the word it read, which is strictly smaller.
//   4. prm_cc_flatten_kernel   label[v] = root(v)
//   5. prm_cc_count_kernel     count[label[v]] += 1: lanes that share the wave's first label add once, the others one each
//   6. prm_cc_summary_kernel   size[v] = count[label[v]]; the roots counted by ballot and the largest (size, lowest label) reduced
//                              across the wave: one atomic each per wave
// No thread waits for another: every loop is a find whose index strictly decreases, or a swap retried from a strictly smaller
// root.  No flag is spun on, no grid barrier, no convergence loop on the host; the six launches do not depend on the graph.
// parent[] is shared across XCDs while kernels 3 and 4 run, and the per-XCD L2s are not coherent for plain accesses: every read
// of parent there is a relaxed agent-scope atomic load, every write an agent-scope atomic (the swap, a relaxed store for halving).
// Under an `alive` mask (prune's second stage) a dead milestone is a root nobody links and no entry with a dead end hooks.
//
// Prune: the keep mask scanned into new_index (rocPRIM, prm_reval_scan), entry flags keep[row] && keep[nbr], their scan, then
// the kept entries moved with new_index[nbr] written in place of nbr, the new offsets, and the states moved row by row (AoS
// [n][dim], binary64 and its binary32 shadow) -- all into second buffers the host swaps in.  Survivors keep their order.
// No kernel of this file uses LDS or scratch; every workgroup has 256 threads.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "oxhip_internal.hpp"
#include "rrt_device.hpp"
#include "prm_csr.hpp"

namespace oxhip {

namespace {

// root of x with path halving; the index read next is always strictly smaller than the one before
__device__ __forceinline__ uint32_t cc_find(uint32_t* parent, uint32_t x) {
    uint32_t p = ld_l2(parent + x);
    while (p != x) {
        const uint32_t g = ld_l2(parent + p);
        if (g != p) st_l2(parent + x, g);   // g is an ancestor of x and g < p < x: x stays in its tree, parent[x] < x stays true
        x = p;
        p = g;
    }
    return x;
}

__device__ __forceinline__ bool cc_live(const uint8_t* __restrict__ alive, uint32_t i) { return alive == nullptr || alive[i] != 0; }

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// components

__global__ __launch_bounds__(256) void prm_cc_self_kernel(uint32_t n, uint32_t* __restrict__ parent, uint32_t* __restrict__ count,
                                                           unsigned long long* __restrict__ summary) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v < n) { parent[v] = v; count[v] = 0; }
    if (v < kCcSummaryWords) summary[v] = 0ull;
}

__global__ __launch_bounds__(256) void prm_cc_init_kernel(const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ nbrs,
                                                           const uint8_t* __restrict__ alive, uint32_t n, uint32_t n_entries, uint32_t* parent) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    bool take = false;
    uint32_t v = 0xFFFFFFFFu, u = 0;
    if (t < n_entries) {
        u = nbrs[t];
        v = row_of(offsets, n, (uint32_t)t);
        take = u < v && cc_live(alive, u) && cc_live(alive, v);
    }
    // the entries of a row are consecutive lanes: a lane heads a run when the lane below holds another row
    const uint32_t below_row = (uint32_t)__shfl_up((int)v, 1, 64);
    const uint64_t heads = __ballot(lane == 0 || below_row != v), takes = __ballot(take);
    if (!take) return;
    const uint32_t run0 = 63u - (uint32_t)__clzll(heads & (below_mask(lane) | (1ull << lane)));   // (lane 0 is a head: never empty)
    const uint64_t earlier = takes & below_mask(lane) & ~below_mask(run0);
    if (earlier == 0) atomicMin(&parent[v], u);   // the first taking lane of the run holds the smallest u of the run
}

__global__ __launch_bounds__(256) void prm_cc_hook_kernel(const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ nbrs,
                                                           const uint8_t* __restrict__ alive, uint32_t n, uint32_t n_entries, uint32_t* parent) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_entries) return;
    const uint32_t u = nbrs[t], v = row_of(offsets, n, (uint32_t)t);
    if (u >= v || !cc_live(alive, u) || !cc_live(alive, v)) return;
    uint32_t a = cc_find(parent, u), b = cc_find(parent, v);
    while (a != b) {
        const uint32_t big = a > b ? a : b, small = a > b ? b : a;
        uint32_t seen = big;
        if (__hip_atomic_compare_exchange_strong(parent + big, &seen, small, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
        // big was linked by somebody else meanwhile: seen = its parent < big.  Both finds start below big.
        a = cc_find(parent, seen);
        b = cc_find(parent, small);
    }
}

__global__ __launch_bounds__(256) void prm_cc_flatten_kernel(uint32_t n, uint32_t* parent, uint32_t* __restrict__ label) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v < n) label[v] = cc_find(parent, v);
}

__global__ __launch_bounds__(256) void prm_cc_count_kernel(const uint32_t* __restrict__ label, const uint8_t* __restrict__ alive, uint32_t n,
                                                            uint32_t* count) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    const bool act = v < n && cc_live(alive, v);
    const uint64_t acts = __ballot(act);
    if (acts == 0) return;
    const uint32_t l = act ? label[v] : 0xFFFFFFFFu;
    const uint32_t first = (uint32_t)__shfl((int)l, (int)__builtin_ctzll(acts), 64);
    const uint64_t same = __ballot(act && l == first);
    if (act && l == first) {
        if ((same & below_mask(threadIdx.x & 63)) == 0) atomicAdd(&count[first], (uint32_t)__popcll(same));
    } else if (act) {
        atomicAdd(&count[l], 1u);
    }
}

// summary[kCcBest] = max over the roots of (size << 32) | (0xFFFFFFFF - label): the largest size, ties to the lowest label
__global__ __launch_bounds__(256) void prm_cc_summary_kernel(const uint32_t* __restrict__ label, const uint32_t* __restrict__ count,
                                                              const uint8_t* __restrict__ alive, uint32_t n, uint32_t* __restrict__ size,
                                                              unsigned long long* summary) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    bool root = false;
    unsigned long long key = 0ull;
    if (v < n) {
        const uint32_t l = label[v], c = count[l];
        size[v] = cc_live(alive, v) ? c : 0u;
        root = l == v && cc_live(alive, v);
        if (root) key = ((unsigned long long)c << 32) | (0xFFFFFFFFu - v);
    }
    const uint64_t roots = __ballot(root);
    if (roots == 0) return;
    const unsigned long long best = wave_max_u64(key);
    if (lane == 0) {
        atomicAdd(&summary[kCcRoots], (unsigned long long)__popcll(roots));
        atomicMax(&summary[kCcBest], best);
    }
}

// ------------------------------------------------------------------------------------------------
// prune: the masks

// stage 1: keep[i] = (valid == nullptr || valid[i]) && (mask == nullptr || mask[i]); *kept counts the ones
__global__ __launch_bounds__(256) void prm_prune_stage1_kernel(const uint8_t* __restrict__ valid, const uint8_t* __restrict__ mask, uint32_t n,
                                                                uint8_t* __restrict__ keep, uint32_t* kept) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    bool k = false;
    if (i < n) {
        k = (valid == nullptr || valid[i] != 0) && (mask == nullptr || mask[i] != 0);
        keep[i] = k ? 1 : 0;
    }
    const uint64_t bal = __ballot(k);
    if (bal != 0 && (threadIdx.x & 63) == 0) atomicAdd(kept, (uint32_t)__popcll(bal));
}

// stage 2, on the components of the stage-1 survivors: min_size (0: not asked) and the largest component (only_label
// 0xFFFFFFFF: not asked; otherwise read from the summary on the device, no read-back in between)
__global__ __launch_bounds__(256) void prm_prune_stage2_kernel(const uint32_t* __restrict__ label, const uint32_t* __restrict__ count,
                                                                const unsigned long long* __restrict__ summary, uint32_t n, uint32_t min_size,
                                                                uint32_t largest, uint8_t* keep, uint32_t* kept) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    bool k = false;
    if (i < n && keep[i] != 0) {
        const uint32_t l = label[i];
        k = count[l] >= min_size && (largest == 0 || l == 0xFFFFFFFFu - (uint32_t)summary[kCcBest]);
        keep[i] = k ? 1 : 0;
    }
    const uint64_t bal = __ballot(k);
    if (bal != 0 && (threadIdx.x & 63) == 0) atomicAdd(kept, (uint32_t)__popcll(bal));
}

// ------------------------------------------------------------------------------------------------
// prune: the compaction.  pos = exclusive scan of keep (milestones), epos = exclusive scan of ekeep (entries).

// new_index[i] = pos[i] or -1; ekeep[e] = keep[row of e] && keep[nbrs[e]]
__global__ __launch_bounds__(256) void prm_prune_flags_kernel(const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ nbrs,
                                                               const uint8_t* __restrict__ keep, const uint32_t* __restrict__ pos, uint32_t n,
                                                               uint32_t n_entries, int32_t* __restrict__ new_index, uint8_t* __restrict__ ekeep) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n) new_index[t] = keep[t] ? (int32_t)pos[t] : -1;
    if (t < n_entries) ekeep[t] = keep[nbrs[t]] != 0 && keep[row_of(offsets, n, (uint32_t)t)] != 0 ? 1 : 0;
}

// the kept entries, renumbered, in their old order (rows stay ascending: new_index is monotone); the offsets of the kept rows
// and the closing offset.  n_entries > 0; offsets_out holds n_kept + 1 words.
__global__ __launch_bounds__(256) void prm_prune_entries_kernel(const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ nbrs,
                                                                 const uint8_t* __restrict__ ekeep, const uint32_t* __restrict__ epos,
                                                                 const int32_t* __restrict__ new_index, uint32_t n, uint32_t n_entries,
                                                                 uint32_t n_kept, uint32_t* __restrict__ offsets_out, uint32_t* __restrict__ nbrs_out) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n_entries && ekeep[t]) nbrs_out[epos[t]] = (uint32_t)new_index[nbrs[t]];
    if (t <= n) {
        const uint32_t total = epos[n_entries - 1] + ekeep[n_entries - 1];
        const uint32_t o = offsets[t];
        const uint32_t before = o < n_entries ? epos[o] : total;   // kept entries in front of row t
        if (t == n) offsets_out[n_kept] = total;
        else if (new_index[t] >= 0) offsets_out[new_index[t]] = before;
    }
}

// one thread per coordinate of a milestone: row i of ms (and of its binary32 shadow, when there is one) to row new_index[i]
__global__ __launch_bounds__(256) void prm_prune_states_kernel(const double* __restrict__ ms, const float* __restrict__ ms32,
                                                                const int32_t* __restrict__ new_index, uint32_t n, uint32_t dim,
                                                                double* __restrict__ ms_out, float* __restrict__ ms32_out) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint64_t)n * dim) return;
    const uint32_t i = (uint32_t)(t / dim), k = (uint32_t)(t - (uint64_t)i * dim);
    const int32_t to = new_index[i];
    if (to < 0) return;
    ms_out[(size_t)to * dim + k] = ms[t];
    if (ms32 != nullptr) ms32_out[(size_t)to * dim + k] = ms32[t];
}

// ------------------------------------------------------------------------------------------------
// launchers.  Every grid has at least one block, so the number of launches does not depend on the graph.

static uint32_t blocks_for(uint64_t work) { return work ? (uint32_t)((work + 255) / 256) : 1u; }

uint32_t launch_prm_components(const uint32_t* offsets, const uint32_t* nbrs, const uint8_t* alive, uint32_t n, uint32_t n_entries,
                               const PrmCcBuffers& b, hipEvent_t after_hook, hipEvent_t after_flatten, hipStream_t s) {
    const dim3 rows(blocks_for(n)), entries(blocks_for(n_entries)), wg(256);
    hipLaunchKernelGGL(prm_cc_self_kernel, rows, wg, 0, s, n, b.parent, b.count, b.summary);
    hipLaunchKernelGGL(prm_cc_init_kernel, entries, wg, 0, s, offsets, nbrs, alive, n, n_entries, b.parent);
    hipLaunchKernelGGL(prm_cc_hook_kernel, entries, wg, 0, s, offsets, nbrs, alive, n, n_entries, b.parent);
    if (after_hook) (void)hipEventRecord(after_hook, s);
    hipLaunchKernelGGL(prm_cc_flatten_kernel, rows, wg, 0, s, n, b.parent, b.label);
    if (after_flatten) (void)hipEventRecord(after_flatten, s);
    hipLaunchKernelGGL(prm_cc_count_kernel, rows, wg, 0, s, b.label, alive, n, b.count);
    hipLaunchKernelGGL(prm_cc_summary_kernel, rows, wg, 0, s, b.label, b.count, alive, n, b.size, b.summary);
    return kCcLaunches;
}

void launch_prm_prune_stage1(const uint8_t* valid, const uint8_t* mask, uint32_t n, uint8_t* keep, uint32_t* kept, hipStream_t s) {
    hipLaunchKernelGGL(prm_prune_stage1_kernel, dim3(blocks_for(n)), dim3(256), 0, s, valid, mask, n, keep, kept);
}

void launch_prm_prune_stage2(const PrmCcBuffers& b, uint32_t n, uint32_t min_size, bool largest, uint8_t* keep, uint32_t* kept, hipStream_t s) {
    hipLaunchKernelGGL(prm_prune_stage2_kernel, dim3(blocks_for(n)), dim3(256), 0, s, b.label, b.count, b.summary, n, min_size,
                       largest ? 1u : 0u, keep, kept);
}

void launch_prm_prune_flags(const uint32_t* offsets, const uint32_t* nbrs, const uint8_t* keep, const uint32_t* pos, uint32_t n,
                            uint32_t n_entries, int32_t* new_index, uint8_t* ekeep, hipStream_t s) {
    const uint64_t work = n_entries > n ? n_entries : n;
    hipLaunchKernelGGL(prm_prune_flags_kernel, dim3(blocks_for(work)), dim3(256), 0, s, offsets, nbrs, keep, pos, n, n_entries, new_index, ekeep);
}

void launch_prm_prune_entries(const uint32_t* offsets, const uint32_t* nbrs, const uint8_t* ekeep, const uint32_t* epos, const int32_t* new_index,
                              uint32_t n, uint32_t n_entries, uint32_t n_kept, uint32_t* offsets_out, uint32_t* nbrs_out, hipStream_t s) {
    if (n_entries == 0) return;   // (the host zeroes the offsets of a roadmap without entries)
    const uint64_t work = n_entries > (uint64_t)n + 1 ? n_entries : (uint64_t)n + 1;
    hipLaunchKernelGGL(prm_prune_entries_kernel, dim3(blocks_for(work)), dim3(256), 0, s, offsets, nbrs, ekeep, epos, new_index, n, n_entries,
                       n_kept, offsets_out, nbrs_out);
}

void launch_prm_prune_states(const double* ms, const float* ms32, const int32_t* new_index, uint32_t n, uint32_t dim, double* ms_out,
                             float* ms32_out, hipStream_t s) {
    hipLaunchKernelGGL(prm_prune_states_kernel, dim3(blocks_for((uint64_t)n * dim)), dim3(256), 0, s, ms, ms32, new_index, n, dim, ms_out, ms32_out);
}

}  // namespace oxhip
