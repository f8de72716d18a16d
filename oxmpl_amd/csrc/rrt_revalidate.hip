// rrt_revalidate.hip -- the trees of an RRT batch re-checked against the obstacles as they stand now, pruned and compacted in
// place (oxhip_rrt_batch_revalidate_trees), on gfx950 (wave64).  The semantics are this build's own; the
// reference has no such call.  Written once over SeqSpace<DIM> (seq_space.hpp): DIM = 1..8 is R^DIM, DIM = 0 is SO(3), DIM = -1 is SO(2).
//
//   1. rrt_reval_edge_kernel<DIM>     R^n and SO(2), one thread per (problem, node i >= 1): check_motion(from = node parent[i], to = node i)
//        by SeqSpace<DIM>::motion_valid -- a motion of any length, the verdict of oxhip_rrt_batch_check_motion on the same two
//        rows.  The tree is SoA [P][dim][cap]: a thread's own node loads coalesced, its parent is a gather.  Writes the verdict
//        byte and the jump pointer of step 2: the parent for a valid edge, -1 for a failed one, 0 for the root.
//        SO(3): a new kernel around so3_motion_valid_seq (or around rrt_so3.hip's wave function) keeps exec masks of that
//        function in spilled SGPRs, as DESIGN.md section 20 found.  So the edges go through the kernel behind
//        oxhip_rrt_batch_check_motion itself (so3_check_motion_kernel, rrt_so3.hip), a bounded chunk at a time:
//        rrt_reval_stage_kernel gathers the chunk's (parent, node) rows, rrt_reval_unstage_kernel turns its verdicts into the
//        verdict bytes and jump pointers.  The staging rows are the 6 bytes per slot the workspace has left, not a tree copy.
//   2. rrt_reval_survive_kernel       one workgroup per problem, pointer jumping in place: jump[i] is always either an ancestor
//        of i reached over valid edges only, or -1 (a failed edge lies between i and the root).  A round replaces jump[i] = j > 0
//        by jump[j], which is a proper ancestor of j (parents precede children) or -1: every value strictly descends, whatever
//        the other threads have or have not written yet, so the loop ends with every pointer at 0 (alive) or -1 -- exact for a
//        chain as deep as the tree, in about log2(depth) rounds.
//   3. rrt_reval_scan_kernel          one workgroup per problem, tiles of 256 nodes with a carry: new_index[i] = survivors below
//        i, -1 for a removed node; the survivor count.
//   4. rrt_reval_compact_kernel<DIM>  one workgroup per problem, in place.  Destinations never exceed sources, the workgroup
//        takes the tiles in ascending order and reads a tile completely (a barrier) before it writes it: a write of tile t lands
//        in tile t or below, where everything has been read already.  Parents are remapped through new_index; the lowest
//        surviving index >= 1 whose state satisfies the goal (SeqSpace::goal_measure against goal_thr) becomes goal_node; the
//        problem's state record is rewritten (n_nodes, goal_node, stop_reason; counters and the RNG position stay).
//      rrt_reval_skip_kernel<DIM>     a node that was unflagged stays unflagged; for every flagged survivor its wave searches
//        the surviving nodes below it for equal coordinates (64 per pass, coalesced) and clears the flag when there is none.
// Workspace: 10 bytes per node slot (verdict byte, survival byte, new index, jump pointer); no second copy of the coordinates.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "oxhip_internal.hpp"
#include "rrt_device.hpp"
#include "seq_space.hpp"

namespace oxhip {

// the words threads of one workgroup hand each other through memory (step 2)
__device__ __forceinline__ int32_t jump_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void jump_store(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// ------------------------------------------------------------------------------------------------
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

// SO(3): slot g of the flattened (problem, node) range -> its rows for so3_check_motion_kernel.  A slot without an edge (the root,
// a slot past the tree, a parent index no tree can hold) stages the root against itself; its verdict is not read.
__device__ __forceinline__ bool reval_slot_edge(const RevalArgs& a, uint64_t g, uint32_t& prob, uint32_t& i, int32_t& par) {
    const uint32_t span = a.tiles * 256u;
    prob = (uint32_t)(g / span);
    i = (uint32_t)(g % span);
    par = -1;
    if (i == 0 || i >= a.state[prob].n_nodes) return false;
    par = a.parent[(size_t)prob * a.cap + i];
    return par >= 0 && (uint32_t)par < i;
}

__global__ __launch_bounds__(256) void rrt_reval_stage_kernel(RevalArgs a, uint64_t g0, uint32_t m) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= m) return;
    uint32_t prob, i;
    int32_t par;
    const bool edge = reval_slot_edge(a, g0 + t, prob, i, par);
    const size_t cap = a.cap;
    const double* tree = a.tree + (size_t)prob * 4 * cap;
    const uint32_t to = edge ? i : 0u, from = edge ? (uint32_t)par : 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        a.stage_from[(size_t)t * 4 + k] = tree[(size_t)k * cap + from];
        a.stage_to[(size_t)t * 4 + k] = tree[(size_t)k * cap + to];
    }
}

__global__ __launch_bounds__(256) void rrt_reval_unstage_kernel(RevalArgs a, uint64_t g0, uint32_t m) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= m) return;
    uint32_t prob, i;
    int32_t par;
    const bool edge = reval_slot_edge(a, g0 + t, prob, i, par);
    if (i >= a.state[prob].n_nodes) return;
    const uint8_t ok = i == 0 ? 1 : (edge && a.stage_out[t] != 0 ? 1 : 0);
    a.edge_ok[(size_t)prob * a.cap + i] = ok;
    a.jump[(size_t)prob * a.cap + i] = i == 0 ? 0 : (ok ? par : -1);
}

// ------------------------------------------------------------------------------------------------
// 2. survival

__global__ __launch_bounds__(256) void rrt_reval_survive_kernel(RevalArgs a) {
    const uint32_t prob = blockIdx.x, n = a.state[prob].n_nodes;
    const size_t base = (size_t)prob * a.cap;
    int32_t* jump = a.jump + base;
    for (;;) {
        bool pending = false;
        for (uint32_t i = threadIdx.x; i < n; i += 256u) {   // jump[i] has one writer: this thread
            const int32_t j = jump_load(jump + i);
            if (j > 0) {
                const int32_t jj = jump_load(jump + j);
                jump_store(jump + i, jj);
                pending = pending || jj > 0;
            }
        }
        if (!__syncthreads_or(pending ? 1 : 0)) break;
    }
    for (uint32_t i = threadIdx.x; i < n; i += 256u) a.alive[base + i] = jump_load(jump + i) == 0 ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------
// 3. scan

__global__ __launch_bounds__(256) void rrt_reval_scan_kernel(RevalArgs a) {
    __shared__ uint32_t wave_sum[4];
    const uint32_t prob = blockIdx.x, n = a.state[prob].n_nodes;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const size_t base = (size_t)prob * a.cap;
    uint32_t carry = 0;
    for (uint32_t t0 = 0; t0 < n; t0 += 256u) {
        const uint32_t i = t0 + threadIdx.x;
        const bool alive = i < n && a.alive[base + i] != 0;
        const uint64_t bal = __ballot(alive);
        if (lane == 0) wave_sum[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t below = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4u; ++w) {
            const uint32_t c = wave_sum[w];
            below += w < wave ? c : 0u;
            total += c;
        }
        if (i < n) a.new_index[base + i] = alive ? (int32_t)(carry + below + (uint32_t)__popcll(bal & below_mask(lane))) : -1;
        carry += total;
        __syncthreads();   // (the next tile's sums overwrite these)
        if (t0 + 256u < t0) break;
    }
    if (threadIdx.x == 0) a.n_after[prob] = carry;
}

// ------------------------------------------------------------------------------------------------
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

// ------------------------------------------------------------------------------------------------
// launchers

void launch_rrt_reval_edges(const DevParams& p, const RevalArgs& a, uint32_t n_problems, hipStream_t s) {
    if (p.space == OXHIP_SPACE_SO3) {
        const uint64_t total = (uint64_t)n_problems * a.tiles * 256u;
        for (uint64_t g0 = 0; g0 < total; g0 += a.stage_cap) {
            const uint32_t m = (uint32_t)(total - g0 < a.stage_cap ? total - g0 : a.stage_cap);
            hipLaunchKernelGGL(rrt_reval_stage_kernel, dim3((m + 255u) / 256u), dim3(256), 0, s, a, g0, m);
            launch_so3_check_motion(p, a.stage_from, a.stage_to, m, a.stage_out, s);
            hipLaunchKernelGGL(rrt_reval_unstage_kernel, dim3((m + 255u) / 256u), dim3(256), 0, s, a, g0, m);
        }
        return;
    }
    space_dispatch<1, true>(p.space, p.dim, [&](auto d) {
        constexpr int D = decltype(d)::value;
        if constexpr (D != 0)   // (SO(3) went through the staging above: no edge kernel exists over it)
            hipLaunchKernelGGL(rrt_reval_edge_kernel<D>, dim3(n_problems * a.tiles), dim3(256), 0, s, SeqSpace<D>::checker(p), a);
    });
}
void launch_rrt_reval_survive(const RevalArgs& a, uint32_t n_problems, hipStream_t s) {
    hipLaunchKernelGGL(rrt_reval_survive_kernel, dim3(n_problems), dim3(256), 0, s, a);
}
void launch_rrt_reval_scan(const RevalArgs& a, uint32_t n_problems, hipStream_t s) {
    hipLaunchKernelGGL(rrt_reval_scan_kernel, dim3(n_problems), dim3(256), 0, s, a);
}
void launch_rrt_reval_compact(const DevParams& p, const RevalArgs& a, uint32_t n_problems, hipStream_t s) {
    space_dispatch<1, true>(p.space, p.dim, [&](auto d) {
        constexpr int D = decltype(d)::value;
        hipLaunchKernelGGL(rrt_reval_compact_kernel<D>, dim3(n_problems), dim3(256), 0, s, a);
        hipLaunchKernelGGL(rrt_reval_skip_kernel<D>, dim3(n_problems * a.tiles), dim3(256), 0, s, a);
    });
}

}  // namespace oxhip
