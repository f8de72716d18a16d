// rrt_reval_kernels.hpp -- the kernels of the RRT re-check that are written over SeqSpace<DIM> (rrt_revalidate.hip's header describes
// them: steps 1 and 4).  rrt_revalidate.hip instantiates them for R^n and SO(3); rrt_so2_services.hip for SO(2).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "oxhip_internal.hpp"
#include "rrt_device.hpp"
#include "seq_space.hpp"

namespace oxhip {

// 1. edge verdicts.  Block b: problem b / tiles, nodes (b % tiles) * 256 ..
template <int DIM>
__global__ __launch_bounds__(256) void rrt_reval_edge_kernel(typename SeqSpace<DIM>::Checker p, RevalArgs a) {
    using Space = SeqSpace<DIM>;
    constexpr int W = Space::W;
    const uint32_t prob = blockIdx.x / a.tiles, i = (blockIdx.x % a.tiles) * 256u + threadIdx.x;
    if (i >= a.state[prob].n_nodes) return;
    // everything the thread needs after the motion check is held in VGPRs (its own output addresses): the checker's tables take
    // the scalar registers (seq_space.hpp, vgpr_pointers)
    size_t cap = a.cap;
    const size_t base = (size_t)prob * cap;
    uint8_t* ok_out = a.edge_ok + base + i;
    int32_t* jump_out = a.jump + base + i;
    const double* node = a.tree + base * W + i;
    asm volatile("" : "+v"(ok_out), "+v"(jump_out), "+v"(node), "+v"(cap));
    // no branch around the check (a saved exec mask is a scalar register pair): the root, and a parent index no tree can hold,
    // check the node against itself and drop the verdict
    const int32_t par = a.parent[base + i];
    // (set_tree and the planners keep parents below their children); the flag waits in a VGPR, not as a lane mask
    uint32_t edge = i > 0 && par >= 0 && (uint32_t)par < i ? 1u : 0u;
    const double* up = node - i + (edge ? (uint32_t)par : i);
    asm volatile("" : "+v"(edge));
    double from[W], to[W];
#pragma unroll
    for (int k = 0; k < W; ++k) { to[k] = node[(size_t)k * cap]; from[k] = up[(size_t)k * cap]; }
    // a planted node may lie outside the bounds: the filter's margin with this motion's ends in play (the verdict does not depend on it)
    const double filt = Space::motion_margin(a.filt_base, from, to);
    typename Space::Checker q = Space::vgpr_pointers(p);
    asm volatile("" : "+v"(q.res));   // (read once, by a division: R^8's last scalar pair)
    const bool valid = Space::motion_valid(q, from, to, filt);
    const uint8_t ok = i == 0 ? 1 : (uint8_t)(edge & (valid ? 1u : 0u));
    const int32_t jump = i == 0 ? 0 : (ok ? par : -1);
    *ok_out = ok;
    *jump_out = jump;
}

// 4. compaction in place, parents remapped, the goal node, the state record
template <int DIM>
__global__ __launch_bounds__(256) void rrt_reval_compact_kernel(RevalArgs a) {
    using Space = SeqSpace<DIM>;
    constexpr int W = Space::W;
    __shared__ uint32_t goal_min;
    const uint32_t prob = blockIdx.x, n = a.state[prob].n_nodes;
    const size_t cap = a.cap, base = (size_t)prob * cap;
    double* tree = a.tree + base * W;
    int32_t* parent = a.parent + base;
    uint8_t* skip = a.skip + base;
    const int32_t* new_index = a.new_index + base;
    double goal[W];
#pragma unroll
    for (int k = 0; k < W; ++k) goal[k] = a.goal_c[(size_t)prob * W + k];
    const double thr = a.goal_thr[prob];
    if (threadIdx.x == 0) goal_min = 0xFFFFFFFFu;
    uint32_t best = 0xFFFFFFFFu;
    for (uint32_t t0 = 0; t0 < n; t0 += 256u) {
        const uint32_t i = t0 + threadIdx.x;
        int32_t d = -1, par = -1;
        uint8_t sk = 0;
        double s[W];
#pragma unroll
        for (int k = 0; k < W; ++k) s[k] = 0.0;
        if (i < n) d = new_index[i];
        if (d >= 0) {
#pragma unroll
            for (int k = 0; k < W; ++k) s[k] = tree[(size_t)k * cap + i];
            par = parent[i];
            sk = skip[i];
        }
        __syncthreads();   // the tile is read: its writes may land anywhere in it
        if (d >= 0) {
            if ((uint32_t)d != i) {   // (d == i: nothing below was removed, the slot already holds all of this)
#pragma unroll
                for (int k = 0; k < W; ++k) tree[(size_t)k * cap + (uint32_t)d] = s[k];
                parent[d] = par >= 0 ? new_index[par] : -1;
                skip[d] = sk;
            }
            if (d >= 1 && Space::goal_measure(s, goal) <= thr) best = best < (uint32_t)d ? best : (uint32_t)d;
        }
        if (t0 + 256u < t0) break;
    }
    if (best != 0xFFFFFFFFu) atomicMin(&goal_min, best);
    __syncthreads();
    if (threadIdx.x == 0) {
        ProblemState st = a.state[prob];
        const uint32_t kept = a.n_after[prob];
        const int32_t new_goal = goal_min == 0xFFFFFFFFu ? -1 : (int32_t)goal_min;
        a.goal_lost[prob] = (st.goal_node >= 0 && (uint32_t)st.goal_node < n && new_goal < 0) ? 1 : 0;
        a.n_removed[prob] = n - kept;
        st.n_nodes = kept;
        st.goal_node = new_goal;
        st.stop_reason = OXHIP_STOP_NONE;
        a.state[prob] = st;
    }
}

// the skip flags of the compacted tree (n_after nodes): block b as in step 1
template <int DIM>
__global__ __launch_bounds__(256) void rrt_reval_skip_kernel(RevalArgs a) {
    constexpr int W = SeqSpace<DIM>::W;
    const uint32_t prob = blockIdx.x / a.tiles, i = (blockIdx.x % a.tiles) * 256u + threadIdx.x;
    const uint32_t n = a.n_after[prob], lane = threadIdx.x & 63u;
    const size_t cap = a.cap, base = (size_t)prob * cap;
    const double* tree = a.tree + base * W;
    uint8_t* skip = a.skip + base;
    uint64_t todo = __ballot(i < n && skip[i] != 0);
    const uint32_t first = i - lane;   // the wave's lane 0
    while (todo != 0) {
        const uint32_t l = (uint32_t)__ffsll((unsigned long long)todo) - 1u;
        todo &= todo - 1;
        const uint32_t node = uni(first + l);
        double c[W];
#pragma unroll
        for (int k = 0; k < W; ++k) c[k] = tree[(size_t)k * cap + node];
        bool found = false;
        for (uint32_t j0 = 0; j0 < node && !found; j0 += 64u) {
            const uint32_t j = j0 + lane;
            bool eq = j < node;
#pragma unroll
            for (int k = 0; k < W; ++k) eq = eq && tree[(size_t)k * cap + (eq ? j : 0u)] == c[k];   // equal as values: -0.0 == +0.0
            found = __ballot(eq) != 0;
        }
        if (!found && lane == l) skip[node] = 0;   // the lower twin was removed: this node can be nearest again
    }
}

}  // namespace oxhip
