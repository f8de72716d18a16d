// prm_shortest.hip -- a batch of PRM queries answered with shortest paths on gfx950 (wave64).  DESIGN.md section 19.
//
// The query sets (start validity, start connections S, goal milestones G) are the flag kernels' of prm_batch.hip, and the rows
// are extracted by its paths kernel; this file holds what lies between:
//   1. prm_shortest_weights_kernel   one thread per CSR entry: w[e] = distance(ms[u], ms[nbrs[e]]), once per roadmap.
//   2. prm_shortest_init_kernel      one thread per (query, milestone): label = distance(start, m) for m in S, +inf elsewhere.
//   3. prm_shortest_labels_kernel    one 1024-thread workgroup per query: the least solution of
//        c[v] = min(init[v], min over neighbours u of fl(c[u] + w(u, v)))
//        by relaxations from a worklist.  A label is the bit pattern of a non-negative binary64, so unsigned order is numeric
//        order and a relaxation is one integer 64-bit atomicMin: the fixed point does not depend on the order of arrival.
//        A node whose label fell enters the next round's worklist once (a stamp word holds the round that claimed it), so a
//        worklist of n words cannot overflow.  The two worklists are the queue and parent rows of the workspace, idle here.
//   4. prm_shortest_levels_kernel    one 1024-thread workgroup per query: breadth-first levels over the tight edges
//        (fl(c[u] + w(u, v)) == c[v]) from the sources (m in S whose label never fell).  A node of the next level keeps the
//        lowest index among its tight predecessors in the current one (atomicMin on its parent word); the first claim enqueues it.
//        hops = the level.  The answer is the goal milestone of least (c, hops, index): two integer reductions in LDS.
// No loop waits on another wave: label rounds and levels are capped at n, and a cap that is hit ends the query with
// OXHIP_ERR_HIP in its status word.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "oxhip_internal.hpp"
#include "rrt_device.hpp"
#include "prm_csr.hpp"
#include "seq_space.hpp"

namespace oxhip {

namespace {

constexpr uint64_t kInfBits = 0x7FF0000000000000ull;   // +inf: no label yet
constexpr uint32_t kUnset = 0xFFFFFFFFu;               // parent / hops of a milestone in no level
constexpr uint32_t kThreads = 1024;

// the 64-bit labels, at L2 like prm_csr.hpp's words
__device__ __forceinline__ uint64_t ld_l2(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint64_t min_l2(uint64_t* p, uint64_t v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ uint64_t add_bits(uint64_t c, double w) {   // fl(c + w): one rounded binary64 add
    return (uint64_t)__double_as_longlong(__longlong_as_double((long long)c) + w);
}

// the space's own distance between two rows (SeqSpace<DIM>::distance: the bits of oxhip_distance_batch / oxhip_so3_op_batch op 0)
template <int DIM>
__device__ __forceinline__ double row_distance(const double* __restrict__ a, const double* __restrict__ b) {
    double x[SeqSpace<DIM>::W], y[SeqSpace<DIM>::W];
    SeqSpace<DIM>::load(a, x);
    SeqSpace<DIM>::load(b, y);
    return SeqSpace<DIM>::distance(x, y);
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// 1. edge weights

template <int DIM>
__global__ __launch_bounds__(256) void prm_shortest_weights_kernel(const double* __restrict__ ms, const uint32_t* __restrict__ offsets,
                                                                   const uint32_t* __restrict__ nbrs, uint32_t n, uint32_t n_entries,
                                                                   double* __restrict__ w) {
    constexpr uint32_t W = SeqSpace<DIM>::W;
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_entries) return;
    const uint32_t u = row_of(offsets, n, e), v = nbrs[e];
    w[e] = row_distance<DIM>(ms + (size_t)u * W, ms + (size_t)v * W);
}

// ------------------------------------------------------------------------------------------------
// 2. initial labels

template <int DIM>
__global__ __launch_bounds__(256) void prm_shortest_init_kernel(PrmBatchArgs b, PrmShortestArgs a) {
    constexpr uint32_t W = SeqSpace<DIM>::W;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const uint32_t c = blockIdx.y;
    if (i >= b.n) return;
    const size_t at = (size_t)c * b.stride + i;
    uint64_t l = kInfBits;
    if (b.flags[at] & 1u) {
        double d = a.mode == 1u ? 1.0 : 0.0;
        if (a.mode == 0u) d = row_distance<DIM>(b.starts + ((size_t)b.q0 + c) * W, b.ms + (size_t)i * W);
        l = (uint64_t)__double_as_longlong(d);
    }
    a.label[at] = l;
    a.stamp[at] = 0u;
}

// ------------------------------------------------------------------------------------------------
// 3. labels

template <int G>
__global__ __launch_bounds__(kThreads) void prm_shortest_labels_kernel(PrmBatchArgs b, PrmShortestArgs a) {
    constexpr uint32_t kGroups = kThreads / G;           // worklist nodes expanded side by side
    __shared__ uint32_t wl_cnt[2];
    __shared__ unsigned long long relaxed;
    const uint32_t tid = threadIdx.x, grp = tid / G, gl = tid % G;
    const uint32_t c = blockIdx.x, n = b.n;
    const uint8_t* __restrict__ flags = b.flags + (size_t)c * b.stride;
    uint64_t* label = a.label + (size_t)c * b.stride;
    uint32_t* stamp = a.stamp + (size_t)c * b.stride;
    uint32_t* wl0 = b.queue + (size_t)c * b.stride;       // the two worklists: rows the levels kernel initialises itself
    uint32_t* wl1 = b.parent + (size_t)c * b.stride;
    const uint32_t* __restrict__ offsets = b.offsets;
    const uint32_t* __restrict__ nbrs = b.nbrs;
    const double* __restrict__ w = a.w;
    const bool use_w = a.mode == 0u;
    const double w_const = a.mode == 1u ? 1.0 : 0.0;

    if (tid == 0) { wl_cnt[0] = 0u; wl_cnt[1] = 0u; relaxed = 0ull; }
    uint32_t rounds = 0, mine = 0;
    bool capped = false;
    if (b.start_valid[c] != 0) {                          // (workgroup-uniform)
        __syncthreads();
        for (uint32_t i = tid; i < n; i += kThreads)      // round 1's worklist: the start connections
            if (flags[i] & 1u) st_l2(wl0 + atomicAdd(&wl_cnt[0], 1u), i);
        uint32_t cur = 0;
        for (;;) {
            __syncthreads();                              // the worklist `cur` is complete
            const uint32_t cnt = wl_cnt[cur];
            if (tid == 0) wl_cnt[cur ^ 1u] = 0u;          // (everyone read it one barrier ago)
            __syncthreads();
            if (cnt == 0) break;
            if (rounds == n) { capped = true; break; }    // every round that lowers a label settles one more node for good
            ++rounds;
            const uint32_t* in = cur ? wl1 : wl0;
            uint32_t* out = cur ? wl0 : wl1;
            for (uint32_t r = grp; r < cnt; r += kGroups) {
                const uint32_t u = ld_l2(in + r);
                const uint64_t cu = ld_l2(label + u);
                const uint32_t e1 = offsets[u + 1];
                for (uint32_t e = offsets[u] + gl; e < e1; e += G) {
                    const uint32_t v = nbrs[e];
                    const uint64_t nb = add_bits(cu, use_w ? w[e] : w_const);
                    ++mine;
                    if (nb < ld_l2(label + v) && nb < min_l2(label + v, nb)) {
                        // this relaxation lowered v: the first to do so in this round puts it on the next worklist
                        if (atomicExch(stamp + v, rounds) != rounds) st_l2(out + atomicAdd(&wl_cnt[cur ^ 1u], 1u), v);
                    }
                }
            }
            cur ^= 1u;
        }
    }
    atomicAdd(&relaxed, (unsigned long long)mine);
    __syncthreads();
    if (tid == 0) {
        a.rounds[c] = rounds;
        a.relaxed[c] = relaxed;
        b.status[c] = capped ? OXHIP_ERR_HIP : OXHIP_OK;  // (the levels kernel writes the query's status)
    }
}

// ------------------------------------------------------------------------------------------------
// 4. tight levels, the answer

template <int G>
__global__ __launch_bounds__(kThreads) void prm_shortest_levels_kernel(PrmBatchArgs b, PrmShortestArgs a) {
    constexpr uint32_t kGroups = kThreads / G;
    __shared__ uint32_t lv_cnt[2], n_start_s, n_goal_s;
    __shared__ unsigned long long best_c, best_hi;
    const uint32_t tid = threadIdx.x, grp = tid / G, gl = tid % G;
    const uint32_t c = blockIdx.x, n = b.n;
    const uint8_t* __restrict__ flags = b.flags + (size_t)c * b.stride;
    const uint64_t* __restrict__ label = a.label + (size_t)c * b.stride;   // final: the labels kernel has ended
    uint32_t* hops = a.stamp + (size_t)c * b.stride;                       // the stamps, read once, become the hops
    uint32_t* parent = b.parent + (size_t)c * b.stride;
    uint32_t* queue = b.queue + (size_t)c * b.stride;
    const uint32_t* __restrict__ offsets = b.offsets;
    const uint32_t* __restrict__ nbrs = b.nbrs;
    const double* __restrict__ w = a.w;
    const bool use_w = a.mode == 0u;
    const double w_const = a.mode == 1u ? 1.0 : 0.0;

    int32_t status = OXHIP_ERR_NO_SOLUTION_FOUND;
    uint32_t path_len = 0, n_start = 0, n_goal = 0;
    int32_t goal_node = -1;
    uint64_t cost = kInfBits;
    if (tid == 0) { lv_cnt[0] = 0u; lv_cnt[1] = 0u; n_start_s = 0u; n_goal_s = 0u; best_c = ~0ull; best_hi = ~0ull; }
    __syncthreads();
    if (b.start_valid[c] == 0) {                          // (workgroup-uniform, as every branch on a result below)
        status = OXHIP_ERR_INVALID_START_STATE;
    } else if (b.status[c] != OXHIP_OK) {
        status = OXHIP_ERR_HIP;                           // the label rounds hit their cap
    } else {
        // ---- level 0: the sources, m in S whose label is still init[m] (no relaxation ever lowered it: its stamp is 0)
        uint32_t cs = 0, cg = 0;
        for (uint32_t i = tid; i < n; i += kThreads) {
            const uint32_t f = flags[i];
            cs += f & 1u;
            cg += (f >> 1) & 1u;
            const bool src = (f & 1u) && ld_l2(hops + i) == 0u;
            st_l2(hops + i, src ? 0u : kUnset);
            st_l2(parent + i, src ? kRoot : kUnset);
            if (src) st_l2(queue + atomicAdd(&lv_cnt[0], 1u), i);
        }
        if (cs) atomicAdd(&n_start_s, cs);
        if (cg) atomicAdd(&n_goal_s, cg);
        // ---- the levels: all of a node's tight predecessors in the level before it compete, the lowest index stays
        uint32_t lev0 = 0, cur = 0, depth = 0;
        bool capped = false;
        for (;;) {
            __syncthreads();                              // level `depth` and its hops are complete
            const uint32_t cnt = lv_cnt[cur];
            if (tid == 0) lv_cnt[cur ^ 1u] = 0u;
            __syncthreads();
            if (cnt == 0) break;
            if (depth == n) { capped = true; break; }     // (levels are disjoint and not empty: unreachable)
            const uint32_t next0 = lev0 + cnt;
            for (uint32_t r = grp; r < cnt; r += kGroups) {
                const uint32_t u = ld_l2(queue + lev0 + r);
                const uint64_t cu = label[u];
                const uint32_t e1 = offsets[u + 1];
                for (uint32_t e = offsets[u] + gl; e < e1; e += G) {
                    const uint32_t v = nbrs[e];
                    const uint64_t nb = add_bits(cu, use_w ? w[e] : w_const);
                    if (nb == label[v] && nb < kInfBits && ld_l2(hops + v) == kUnset) {
                        if (atomicMin(parent + v, u) == kUnset) st_l2(queue + next0 + atomicAdd(&lv_cnt[cur ^ 1u], 1u), v);
                    }
                }
            }
            __syncthreads();                              // the next level is complete
            const uint32_t next_cnt = lv_cnt[cur ^ 1u];
            for (uint32_t t = tid; t < next_cnt; t += kThreads) st_l2(hops + ld_l2(queue + next0 + t), depth + 1u);
            lev0 = next0;
            cur ^= 1u;
            ++depth;
        }
        n_start = n_start_s;
        n_goal = n_goal_s;
        // ---- the goal milestone of least (c, hops, index)
        for (uint32_t i = tid; i < n; i += kThreads)
            if ((flags[i] & 2u) && label[i] < kInfBits) atomicMin(&best_c, (unsigned long long)label[i]);
        __syncthreads();
        const uint64_t bc = best_c;
        if (capped) {
            status = OXHIP_ERR_HIP;
        } else if (bc != ~0ull) {
            for (uint32_t i = tid; i < n; i += kThreads)
                if ((flags[i] & 2u) && label[i] == bc) atomicMin(&best_hi, ((unsigned long long)ld_l2(hops + i) << 32) | i);
            __syncthreads();
            const uint64_t bh = best_hi;
            const uint32_t h = (uint32_t)(bh >> 32);
            if (h == kUnset) {
                status = OXHIP_ERR_HIP;                   // a finite label no tight chain reaches: cannot happen
            } else {
                status = OXHIP_OK;
                goal_node = (int32_t)(uint32_t)bh;
                path_len = h + 2u;                        // the start state, h + 1 milestones
                cost = bc;
            }
        }
    }
    if (tid == 0) {
        b.status[c] = status;
        b.path_len[c] = path_len;
        b.goal_node[c] = goal_node;
        b.n_start[c] = n_start;
        b.n_goal[c] = n_goal;
        a.cost[c] = __longlong_as_double((long long)cost);
    }
}

// ------------------------------------------------------------------------------------------------
// launchers

void launch_prm_shortest_weights(bool so3, uint32_t dim, const double* ms, const uint32_t* offsets, const uint32_t* nbrs, uint32_t n,
                                 uint32_t n_entries, double* w, hipStream_t s) {
    if (n == 0 || n_entries == 0) return;
    space_dispatch(prm_space(so3), dim, [&](auto d) {
        constexpr int D = decltype(d)::value;
        hipLaunchKernelGGL(prm_shortest_weights_kernel<D>, dim3((n_entries + 255) / 256), dim3(256), 0, s, ms, offsets, nbrs, n, n_entries, w);
    });
}

void launch_prm_shortest_init(bool so3, const PrmBatchArgs& b, const PrmShortestArgs& a, hipStream_t s) {
    const dim3 grid(b.n ? (b.n + 255) / 256 : 1, b.n_chunk);
    space_dispatch(prm_space(so3), b.dim, [&](auto d) {
        constexpr int D = decltype(d)::value;
        hipLaunchKernelGGL(prm_shortest_init_kernel<D>, grid, dim3(256), 0, s, b, a);
    });
}

template <int G>
static void launch_search(const PrmBatchArgs& b, const PrmShortestArgs& a, bool levels, hipStream_t s) {
    if (levels) hipLaunchKernelGGL(prm_shortest_levels_kernel<G>, dim3(b.n_chunk), dim3(kThreads), 0, s, b, a);
    else hipLaunchKernelGGL(prm_shortest_labels_kernel<G>, dim3(b.n_chunk), dim3(kThreads), 0, s, b, a);
}

static void launch_search_group(const PrmBatchArgs& b, const PrmShortestArgs& a, uint32_t group, bool levels, hipStream_t s) {
    switch (group) {
        case 4: launch_search<4>(b, a, levels, s); break;
        case 8: launch_search<8>(b, a, levels, s); break;
        case 16: launch_search<16>(b, a, levels, s); break;
        case 32: launch_search<32>(b, a, levels, s); break;
        default: launch_search<64>(b, a, levels, s); break;
    }
}

void launch_prm_shortest_labels(const PrmBatchArgs& b, const PrmShortestArgs& a, uint32_t group, hipStream_t s) {
    launch_search_group(b, a, group, false, s);
}

void launch_prm_shortest_levels(const PrmBatchArgs& b, const PrmShortestArgs& a, uint32_t group, hipStream_t s) {
    launch_search_group(b, a, group, true, s);
}

}  // namespace oxhip
