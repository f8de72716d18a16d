// path_simplify.hip -- the solution paths of a whole RRT / RRTConnect / RRT* batch, extracted and shortcut on gfx950 (wave64).
// DESIGN.md section 18.
//
//   1. path_len_kernel / path_rows_kernel   one wave per problem: reconstruct_path (rrt.rs:118-128, and the splice of
//        rrt_connect.rs:288-304) on the device -- the parent chain from the goal node is counted, the host takes one prefix sum,
//        and the chain is walked again writing the rows reversed behind the problem's offset (what prm_batch_paths_kernel does
//        for a roadmap).  Rows are copied as 64-bit words: bit for bit.
//   2. path_pairs_kernel<D>   (path_kernels.hpp; D = 0: SO(3), D = -1: SO(2), seq_space.hpp; the SO(2) instantiations of this and
//        of the DP live in rrt_so2_services.hip) the hot path: one thread per pair (i, d = j - i), 2 <= d <= span, of
//        a path's own waypoints, check_motion(from = p_i, to = p_j) by SeqSpace<D>::motion_valid (motion_valid_seq<D> /
//        so3_motion_valid_seq), one bit per pair.  The pairs are dealt d-major: slot = (d - 2) * L + i, so the 64 lanes of a
//        wave hold motions of equal index distance -- similar lengths, similar step counts -- and a wave's ballot is one word of
//        the bit matrix (a problem's slots are padded to whole words; slots with i + d >= L are idle).  The motion check's
//        midpoint filter runs over a wave-uniform sphere index (scalar loads); its absolute margin is per motion, since a path
//        state may lie outside the bounds (the goal centre, a tree given through set_tree).
//   3. path_dp_kernel<KIND>  (0: R^n, 1: SO(3), 2: SO(2)) one wave per problem, j serial: cost[j] = min over the window of i with valid(i, j) of
//        fl(cost[i] + distance(p_i, p_j)), lowest i among ties (every lane scans its i ascending with strict '<', then the
//        lexicographic (cost, i) minimum over the wave).  Distances are computed on the fly in the space's own evaluation order,
//        unfused.  Then the parent chain from L - 1 is written out in path order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "oxhip_internal.hpp"
#include "rrt_device.hpp"
#include "seq_space.hpp"
#include "path_kernels.hpp"

namespace oxhip {

constexpr uint32_t kCorruptLen = 0xFFFFFFFFu;   // a chain that leaves the tree or never ends

// ------------------------------------------------------------------------------------------------
// 1. extraction

// walks `parent` from node v; returns the number of nodes met, kCorruptLen when the chain leaves [0, n) or is longer than n
__device__ __forceinline__ uint32_t chain_length(const int32_t* __restrict__ parent, int32_t v, uint32_t n) {
    uint32_t cnt = 0;
    while (v >= 0) {
        if ((uint32_t)v >= n || cnt >= n) return kCorruptLen;
        ++cnt;
        v = parent[v];
    }
    return cnt;
}

__global__ __launch_bounds__(64) void path_len_kernel(DevParams p, PathArgs a) {
    const uint32_t prob = blockIdx.x;
    const ProblemState st = p.state[prob];
    uint32_t la = 0, lb = 0;
    if (st.goal_node >= 0) {
        la = chain_length(p.parent + (size_t)prob * p.cap, st.goal_node, st.n_nodes);
        if (la != kCorruptLen && p.parent_b && st.goal_node_b >= 0) {
            const int32_t* pb = p.parent_b + (size_t)prob * p.cap;
            // the goal path without its first element, the duplicate connection point (rrt_connect.rs:296-301)
            lb = (uint32_t)st.goal_node_b < st.n_nodes_b ? chain_length(pb, pb[st.goal_node_b], st.n_nodes_b) : kCorruptLen;
        }
    }
    if (threadIdx.x == 0) {
        const bool bad = la == kCorruptLen || lb == kCorruptLen;
        a.len_a[prob] = bad ? 0u : la;
        a.len[prob] = bad ? kCorruptLen : la + lb;
    }
}

__global__ __launch_bounds__(64) void path_rows_kernel(DevParams p, PathArgs a) {
    const uint32_t prob = blockIdx.x, lane = threadIdx.x, dim = p.dim;
    const uint32_t len = a.len[prob], la = a.len_a[prob];
    if (len == 0) return;
    const size_t cap = p.cap;
    const uint64_t off = a.off[prob];
    uint64_t* rows = (uint64_t*)a.rows;
    const ProblemState st = p.state[prob];
    {
        const uint64_t* tree = (const uint64_t*)p.tree + (size_t)prob * dim * cap;
        const int32_t* parent = p.parent + (size_t)prob * cap;
        int32_t v = st.goal_node;
        for (uint32_t j = la; j-- > 0;) {                        // every lane walks the chain; lane j % 64 writes row j
            if ((j & 63u) == lane)
                for (uint32_t k = 0; k < dim; ++k) rows[(off + j) * dim + k] = tree[(size_t)k * cap + (uint32_t)v];
            v = parent[v];
        }
    }
    if (len > la) {
        const uint64_t* tree = (const uint64_t*)p.tree_b + (size_t)prob * dim * cap;
        const int32_t* parent = p.parent_b + (size_t)prob * cap;
        int32_t v = parent[st.goal_node_b];
        for (uint32_t j = la; j < len; ++j) {
            if ((j & 63u) == lane)
                for (uint32_t k = 0; k < dim; ++k) rows[(off + j) * dim + k] = tree[(size_t)k * cap + (uint32_t)v];
            v = parent[v];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// launchers

void launch_path_len(const DevParams& p, const PathArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(path_len_kernel, dim3(p.n_problems), dim3(64), 0, s, p, a);
}
void launch_path_rows(const DevParams& p, const PathArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(path_rows_kernel, dim3(p.n_problems), dim3(64), 0, s, p, a);
}

uint64_t path_pair_words(uint32_t L, uint32_t max_span) {
    if (L < 3) return 0;
    const uint32_t full = L - 1u;
    const uint32_t S = max_span == 0u || max_span > full ? full : max_span;
    if (S < 2) return 0;
    return ((uint64_t)(S - 1u) * L + 63u) / 64u;
}

void launch_path_pairs(const DevParams& p, const PairArgs& a, hipStream_t s) {
    if (a.n_words == 0) return;
    const dim3 grid((uint32_t)((a.n_words + 3u) / 4u)), block(256);
    if (p.space == OXHIP_SPACE_SO2) return launch_so2_path_pairs(p, a, s);   // (instantiated in rrt_so2_services.hip)
    space_dispatch<2>(p.space == OXHIP_SPACE_SO3, p.dim, [&](auto d) {   // (an R^n batch has at least two dimensions here: simplify_supported)
        constexpr int D = decltype(d)::value;
        hipLaunchKernelGGL(path_pairs_kernel<D>, grid, block, 0, s, SeqSpace<D>::checker(p), a);
    });
}

void launch_path_dp(const DevParams& p, const PairArgs& a, const SimplifyOut& o, hipStream_t s) {
    if (p.space == OXHIP_SPACE_SO3) hipLaunchKernelGGL(path_dp_kernel<1>, dim3(a.n_chunk), dim3(64), 0, s, a, o, 4u);
    else if (p.space == OXHIP_SPACE_SO2) launch_so2_path_dp(a, o, s);
    else hipLaunchKernelGGL(path_dp_kernel<0>, dim3(a.n_chunk), dim3(64), 0, s, a, o, p.dim);
}

}  // namespace oxhip
