// path_simplify.hip -- the solution paths of a whole RRT / RRTConnect / RRT* batch, extracted on gfx950 (wave64).  DESIGN.md section
// 18; the extracted rows are shortcut where they lie by shortcut_core.hip (m = 1: a waypoint is a row).
//
//   path_len_kernel / path_rows_kernel   one wave per problem: reconstruct_path (rrt.rs:118-128, and the splice of
//        rrt_connect.rs:288-304) on the device -- the parent chain from the goal node is counted, the host takes one prefix sum,
//        and the chain is walked again writing the rows reversed behind the problem's offset (what prm_batch_paths_kernel does
//        for a roadmap).  Rows are copied as 64-bit words: bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "oxhip_internal.hpp"
#include "rrt_device.hpp"

namespace oxhip {

constexpr uint32_t kCorruptLen = 0xFFFFFFFFu;   // a chain that leaves the tree or never ends

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

void launch_path_len(const DevParams& p, const PathArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(path_len_kernel, dim3(p.n_problems), dim3(64), 0, s, p, a);
}
void launch_path_rows(const DevParams& p, const PathArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(path_rows_kernel, dim3(p.n_problems), dim3(64), 0, s, p, a);
}

}  // namespace oxhip
