// path_simplify.hip -- the solution paths of a whole RRT / RRTConnect / RRT* batch, extracted and shortcut on gfx950 (wave64).
// DESIGN.md section 18.
//
//   1. path_len_kernel / path_rows_kernel   one wave per problem: reconstruct_path (rrt.rs:118-128, and the splice of
//        rrt_connect.rs:288-304) on the device -- the parent chain from the goal node is counted, the host takes one prefix sum,
//        and the chain is walked again writing the rows reversed behind the problem's offset (what prm_batch_paths_kernel does
//        for a roadmap).  Rows are copied as 64-bit words: bit for bit.
//   2. path_pairs_kernel<D>   (D = 0: SO(3), D = -1: SO(2), seq_space.hpp) the hot path: one thread per pair (i, d = j - i), 2 <= d <= span, of
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
// 2. the pair matrix

__device__ __forceinline__ uint32_t path_span(uint32_t L, uint32_t max_span) {
    const uint32_t full = L - 1u;
    return max_span == 0u || max_span > full ? full : max_span;
}

// the wave's word gw of the round -> its problem c (woff is ascending; equal neighbours are problems without pairs)
__device__ __forceinline__ uint32_t word_problem(const uint64_t* __restrict__ woff, uint32_t n_chunk, uint64_t gw) {
    uint32_t lo = 0, hi = n_chunk;                               // woff[lo] <= gw < woff[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = uni((lo + hi) >> 1);
        if (uni64(woff[mid]) <= gw) lo = mid; else hi = mid;
    }
    return lo;
}

struct PairSlot {
    uint64_t row_i, row_j;   // rows of the batch
    bool active;
};
__device__ __forceinline__ PairSlot pair_slot(const PairArgs& a, uint64_t gw, uint32_t lane) {
    const uint32_t c = word_problem(a.woff, a.n_chunk, gw);
    const uint32_t prob = a.q0 + c;
    const uint32_t L = uni(a.len[prob]);
    const uint32_t S = path_span(L, a.max_span);
    const uint64_t slot = (gw - uni64(a.woff[c])) * 64u + lane;
    const uint64_t dd = slot / L;                                // d - 2
    const uint32_t i = (uint32_t)(slot - dd * L);
    const uint64_t off = uni64(a.off[prob]);
    PairSlot s;
    s.active = dd + 2u <= S && (uint64_t)i + dd + 2u < L;
    s.row_i = off + i;
    s.row_j = off + i + (s.active ? dd + 2u : 0u);
    return s;
}

template <int D>
__global__ __launch_bounds__(256) void path_pairs_kernel(typename SeqSpace<D>::Checker p, PairArgs a) {
    using Space = SeqSpace<D>;
    const uint64_t gw = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (gw >= a.n_words) return;                                 // wave-uniform
    const uint32_t lane = threadIdx.x & 63u;
    const PairSlot s = pair_slot(a, gw, lane);
    bool ok = false;
    if (s.active) {
        double from[Space::W], to[Space::W];
        Space::load(a.rows + s.row_i * Space::W, from);
        Space::load(a.rows + s.row_j * Space::W, to);
        ok = Space::motion_valid(p, from, to, Space::motion_margin(a.filt_base, from, to));
    }
    const uint64_t word = __ballot(ok);
    if (lane == 0) a.bits[gw] = word;
}

// ------------------------------------------------------------------------------------------------
// 3. the shortest chain over the valid pairs

template <int KIND>
__device__ __forceinline__ double path_distance(const double* __restrict__ rows, uint64_t ri, uint64_t rj, uint32_t dim) {
    if (KIND == 2) return so2_distance(rows[ri], rows[rj]);
    if (KIND == 1) {
        const double x[4] = {rows[ri * 4], rows[ri * 4 + 1], rows[ri * 4 + 2], rows[ri * 4 + 3]};
        const double y[4] = {rows[rj * 4], rows[rj * 4 + 1], rows[rj * 4 + 2], rows[rj * 4 + 3]};
        return so3_distance(x, y);
    }
    double x[kMaxDim], y[kMaxDim];
#pragma unroll
    for (int k = 0; k < kMaxDim; ++k) if (k < (int)dim) { x[k] = rows[ri * dim + k]; y[k] = rows[rj * dim + k]; }
    return sqrt(dist2<kMaxDim>(x, y, (int)dim));
}

// what one lane stores and another loads: the fences keep the compiler from moving either, the memory is the wave's own
__device__ __forceinline__ void wave_publish() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <int KIND>
__global__ __launch_bounds__(64) void path_dp_kernel(PairArgs a, SimplifyOut o, uint32_t dim) {
    const uint32_t c = blockIdx.x, lane = threadIdx.x;
    const uint32_t prob = a.q0 + c;
    const uint32_t L = a.len[prob];
    if (L == 0) {
        if (lane == 0) { o.simp_len[prob] = 0; o.raw_cost[prob] = 0.0; o.simp_cost[prob] = 0.0; o.checks[prob] = 0; }
        return;
    }
    const uint64_t off = a.off[prob];
    const uint32_t S = path_span(L, a.max_span);
    const uint64_t* bits = a.bits + a.woff[c];
    double* cost = o.cost + off;
    uint32_t* par = o.par + off;
    uint32_t* idx = o.idx + off;
    if (lane == 0) { cost[0] = 0.0; par[0] = 0u; }
    wave_publish();
    double raw = 0.0;
    for (uint32_t j = 1; j < L; ++j) {
        Exact best{__builtin_inf(), 0xFFFFFFFFu};
        for (uint32_t i = (j > S ? j - S : 0u) + lane; i < j; i += 64u) {
            const uint32_t d = j - i;
            bool ok = d == 1u;                                   // the planner accepted that edge
            if (!ok) {
                const uint64_t slot = (uint64_t)(d - 2u) * L + i;
                ok = (bits[slot >> 6] >> (slot & 63u)) & 1ull;
            }
            if (ok) {
                const double dij = path_distance<KIND>(a.rows, off + i, off + j, dim);
                const double cand = cost[i] + dij;
                if (cand < best.dist) { best.dist = cand; best.idx = i; }
            }
        }
        const Exact r = exact_wave_reduce(best);
        const double adj = path_distance<KIND>(a.rows, off + j - 1u, off + j, dim);
        raw = raw + adj;
        if (lane == 0) { cost[j] = r.dist; par[j] = r.idx < j ? r.idx : j - 1u; }
        wave_publish();
    }
    // the parent chain from L - 1, in path order
    uint32_t n = 1;
    for (uint32_t v = L - 1u; v != 0u; v = par[v]) ++n;
    uint32_t v = L - 1u;
    for (uint32_t t = n; t-- > 0;) {
        if ((t & 63u) == lane) idx[t] = v;
        v = par[v];
    }
    if (lane == 0) {
        o.simp_len[prob] = n;
        o.raw_cost[prob] = raw;
        o.simp_cost[prob] = cost[L - 1u];
        // pairs with 2 <= d <= S: sum of (L - d)
        o.checks[prob] = S >= 2u ? (uint64_t)(S - 1u) * L - ((uint64_t)S * (S + 1u) / 2u - 1u) : 0ull;
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
    space_dispatch<2, true>(p.space, p.dim, [&](auto d) {   // (an R^n batch has at least two dimensions here: simplify_supported)
        constexpr int D = decltype(d)::value;
        hipLaunchKernelGGL(path_pairs_kernel<D>, grid, block, 0, s, SeqSpace<D>::checker(p), a);
    });
}

void launch_path_dp(const DevParams& p, const PairArgs& a, const SimplifyOut& o, hipStream_t s) {
    if (p.space == OXHIP_SPACE_SO3) hipLaunchKernelGGL(path_dp_kernel<1>, dim3(a.n_chunk), dim3(64), 0, s, a, o, 4u);
    else if (p.space == OXHIP_SPACE_SO2) hipLaunchKernelGGL(path_dp_kernel<2>, dim3(a.n_chunk), dim3(64), 0, s, a, o, 1u);
    else hipLaunchKernelGGL(path_dp_kernel<0>, dim3(a.n_chunk), dim3(64), 0, s, a, o, p.dim);
}

}  // namespace oxhip
