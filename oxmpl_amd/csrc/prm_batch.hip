// prm_batch.hip -- a batch of PRM queries on one roadmap, search included, on gfx950 (wave64).  DESIGN.md section 17.
//
// Reference: oxmpl/src/geometric/planners/prm.rs:243-307 (solve) and :189-208 (reconstruct_path), once per query.
//   1. prm_batch_flags_kernel<DIM>   one thread per (query, milestone): start validity, start connection, goal membership --
//        the lines of prm_query_kernel<DIM> over SeqSpace<DIM> (seq_space.hpp; DIM = 0: SO(3)), so the bits are its; the
//        midpoint filter's absolute margin is per query (the start may lie anywhere).
//   2. prm_batch_search_kernel   one 1024-thread workgroup per query: the reference's FIFO (:270-301) evaluated level by level.
//        Level 0 is the start connections, ascending; a node's rank is its position in its level.  A level that holds goal
//        milestones answers with the one of lowest rank.  Otherwise every unvisited neighbour of the level takes as parent the
//        level's node of minimum rank adjacent to it (atomicMin on a claim word: order of arrival is irrelevant), and the next
//        level is those neighbours ordered by (parent's rank, position in the parent's ascending edge list): a count per parent
//        and a prefix sum.  That is the order in which the FIFO enqueues them, so parents, answer and path are the FIFO's.
//        Integer decisions only.  A node's edge list is striped over a group of G lanes (G ~ the roadmap's mean degree).
//        Per query and milestone: one claim / parent word and one queue word in HBM / L2 next to the flag byte; all levels are
//        disjoint, so one queue of n words holds them back to back; up to 2^18 milestones, a visited bitmap in LDS.
//        Everything a query touches is its own.
//   3. prm_batch_paths_kernel    one wave per query: parents from the goal milestone back to a start connection, written
//        reversed behind the start state at the query's row offset.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "oxhip_internal.hpp"
#include "rrt_device.hpp"
#include "prm_csr.hpp"
#include "seq_space.hpp"

namespace oxhip {

// ------------------------------------------------------------------------------------------------
// 1. flags

template <int DIM>
__global__ __launch_bounds__(256) void prm_batch_flags_kernel(typename SeqSpace<DIM>::Checker p, PrmBatchArgs b, double near) {
    using Space = SeqSpace<DIM>;
    constexpr int W = Space::W;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const uint32_t c = blockIdx.y;                 // query of the round
    const size_t q = (size_t)b.q0 + c;             // query of the batch
    double s[W], g[W];
#pragma unroll
    for (int k = 0; k < W; ++k) { s[k] = b.starts[q * W + k]; g[k] = b.goals[q * W + k]; }
    if (i == 0) b.start_valid[c] = Space::state_valid(p, s) ? 1u : 0u;                       // prm.rs:244
    if (i >= b.n) return;
    double m[W];
    Space::load(b.ms + (size_t)i * W, m);
    // the flag byte as prm_query_kernel writes it (prm_kernels.hip, which says why the lines stand in the kernel); the midpoint
    // filter's absolute margin is per query (R^n: the start may lie anywhere)
    uint8_t f = 0;
    if (Space::connects(s, m, near) && Space::motion_valid(p, s, m, b.filt[q])) f |= 1;     // prm.rs:251-252
    if (Space::goal_measure(m, g) <= b.goal_thr[q]) f |= 2;                                  // goal.is_satisfied, prm.rs:261
    b.flags[(size_t)c * b.stride + i] = f;
}

// ------------------------------------------------------------------------------------------------
// 2. search

// a claim / parent word: 0xFFFFFFFF (what the host's memset leaves) = not yet in a level, then
constexpr uint32_t kTentative = 0x80000000u;   // | rank: claimed in the level being expanded, kRoot (prm_csr.hpp): a start connection
constexpr uint32_t kNoGoal = 0xFFFFFFFFu;


// 1024 threads per query: the search is a chain of dependent loads (edge list -> claim word), and with one workgroup per query
// the waves of that workgroup are all the latency hiding a query has
constexpr uint32_t kSearchThreads = 1024, kSearchWaves = kSearchThreads / 64;

// LDS_VISITED: one bit per milestone that is in a level, in LDS (dynamic, ceil(n / 32) words): most neighbours a level meets are
// already in one, and the bit answers for them without the claim word's trip to L2.  A bit is set with the parent, by the one
// group that owns the node, so a reader that sees it early skips a node it would have dropped at the claim test anyway.
template <int G, bool LDS_VISITED>
__global__ __launch_bounds__(kSearchThreads) void prm_batch_search_kernel(PrmBatchArgs b) {
    constexpr uint32_t kGroups = kSearchThreads / G;     // level nodes expanded side by side
    extern __shared__ uint32_t visited[];
    __shared__ uint32_t w_start[kSearchWaves], w_goal[kSearchWaves], w_tile[kSearchWaves];
    __shared__ uint32_t goal_rank;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t grp = tid / G, gl = tid % G;                  // group of the workgroup, lane of the group
    const uint32_t gshift = lane & ~(uint32_t)(G - 1);           // the group's first lane in its wave
    const uint64_t gmask = (G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull)) << gshift;
    const uint32_t c = blockIdx.x, n = b.n;
    const uint8_t* __restrict__ flags = b.flags + (size_t)c * b.stride;
    uint32_t* parent = b.parent + (size_t)c * b.stride;
    uint32_t* queue = b.queue + (size_t)c * b.stride;
    const uint32_t* __restrict__ offsets = b.offsets;
    const uint32_t* __restrict__ nbrs = b.nbrs;

    int32_t status = OXHIP_ERR_NO_SOLUTION_FOUND;
    uint32_t path_len = 0, n_start = 0, n_goal = 0;
    int32_t goal_node = -1;
    if (b.start_valid[c] == 0) {                                 // prm.rs:243-246 (workgroup-uniform)
        status = OXHIP_ERR_INVALID_START_STATE;
    } else {
        // ---- level 0: the start connections in ascending order; every wave compacts a contiguous slice of the milestones
        if (tid == 0) goal_rank = kNoGoal;
        if (LDS_VISITED)
            for (uint32_t w = tid; w < (n + 31u) / 32u; w += kSearchThreads) visited[w] = 0u;
        const uint32_t slice = ((n + kSearchThreads - 1u) / kSearchThreads) * 64u;   // per wave, a multiple of 64
        const uint32_t i0 = wave * slice, i1 = i0 + slice < n ? i0 + slice : n;
        uint32_t cs = 0, cg = 0;
        for (uint32_t i = i0 + lane; i < i0 + slice; i += 64u) {
            const uint32_t f = i < i1 ? flags[i] : 0u;
            cs += (uint32_t)__popcll(__ballot(f & 1u));
            cg += (uint32_t)__popcll(__ballot(f & 2u));
        }
        if (lane == 0) { w_start[wave] = cs; w_goal[wave] = cg; }
        __syncthreads();
        uint32_t base = 0;
#pragma unroll
        for (uint32_t w = 0; w < kSearchWaves; ++w) {
            base += w < wave ? w_start[w] : 0u;
            n_start += w_start[w];
            n_goal += w_goal[w];
        }
        if (n_start != 0 && n_goal != 0) {                       // else prm.rs:266-268
            for (uint32_t i = i0 + lane; i < i0 + slice; i += 64u) {
                const uint32_t f = i < i1 ? flags[i] : 0u;
                const uint64_t bal = __ballot(f & 1u);
                if (f & 1u) {
                    const uint32_t pos = base + (uint32_t)__popcll(bal & below_mask(lane));
                    st_l2(queue + pos, i);
                    st_l2(parent + i, kRoot);
                    if (LDS_VISITED) atomicOr(&visited[i >> 5], 1u << (i & 31u));
                    if (f & 2u) atomicMin(&goal_rank, pos);
                }
                base += (uint32_t)__popcll(bal);
            }
            // ---- the levels
            uint32_t lev0 = 0, cnt = n_start, depth = 0;         // the level's slice of the queue; edges from a start connection
            for (;;) {
                __syncthreads();
                const uint32_t gr = goal_rank;
                if (gr != kNoGoal) {                             // the first goal milestone the FIFO would dequeue
                    goal_node = (int32_t)ld_l2(queue + lev0 + gr);
                    status = OXHIP_OK;
                    path_len = depth + 2u;                       // the start state, depth + 1 milestones
                    break;
                }
                if (cnt == 0) break;                             // the search ran dry (prm.rs:304)
                // (a) claims: every neighbour not yet in a level keeps the minimum rank that reached it
                for (uint32_t r = grp; r < cnt; r += kGroups) {
                    const uint32_t u = ld_l2(queue + lev0 + r);
                    const uint32_t e1 = offsets[u + 1];
                    const uint32_t claim = kTentative | r;
                    for (uint32_t e = offsets[u] + gl; e < e1; e += G) {
                        const uint32_t v = nbrs[e];
                        if (LDS_VISITED && ((visited[v >> 5] >> (v & 31u)) & 1u)) continue;
                        if (ld_l2(parent + v) > claim) atomicMin(parent + v, claim);
                    }
                }
                __syncthreads();
                // (b) the next level behind this one: per parent in rank order, its claimed neighbours as they stand in its list
                const uint32_t next0 = lev0 + cnt;
                uint32_t next_cnt = 0;
                for (uint32_t t0 = 0; t0 < cnt; t0 += kGroups) {
                    const uint32_t r = t0 + grp;
                    const bool live = r < cnt;
                    const uint32_t claim = kTentative | r;
                    uint32_t u = 0, e0 = 0, e1 = 0, mine = 0;
                    if (live) {
                        u = ld_l2(queue + lev0 + r);
                        e0 = offsets[u];
                        e1 = offsets[u + 1];
                        for (uint32_t e = e0; e < e1; e += G) {
                            bool own = false;
                            if (e + gl < e1) {
                                const uint32_t v = nbrs[e + gl];
                                own = !(LDS_VISITED && ((visited[v >> 5] >> (v & 31u)) & 1u)) && ld_l2(parent + v) == claim;
                            }
                            mine += (uint32_t)__popcll(__ballot(own) & gmask);
                        }
                    }
                    // exclusive scan of the groups' counts over the workgroup
                    uint32_t x = gl == 0 ? mine : 0u;
                    uint32_t inc = x;
#pragma unroll
                    for (int off = 1; off < 64; off <<= 1) {
                        const uint32_t o = __shfl_up(inc, off, 64);
                        if ((int)lane >= off) inc += o;
                    }
                    if (lane == 63) w_tile[wave] = inc;
                    __syncthreads();
                    uint32_t pre = 0, total = 0;
#pragma unroll
                    for (uint32_t w = 0; w < kSearchWaves; ++w) {
                        pre += w < wave ? w_tile[w] : 0u;
                        total += w_tile[w];
                    }
                    uint32_t at = next0 + next_cnt + pre + __shfl(inc - x, (int)gshift, 64);   // the group leader's exclusive prefix
                    if (live) {
                        for (uint32_t e = e0; e < e1; e += G) {
                            uint32_t v = 0;
                            bool own = false;
                            if (e + gl < e1) {
                                v = nbrs[e + gl];
                                own = !(LDS_VISITED && ((visited[v >> 5] >> (v & 31u)) & 1u)) && ld_l2(parent + v) == claim;
                            }
                            const uint64_t bal = __ballot(own) & gmask;
                            if (own) {
                                const uint32_t pos = at + (uint32_t)__popcll(bal & below_mask(lane));
                                st_l2(queue + pos, v);
                                st_l2(parent + v, u);
                                if (LDS_VISITED) atomicOr(&visited[v >> 5], 1u << (v & 31u));
                                if (flags[v] & 2u) atomicMin(&goal_rank, pos - next0);
                            }
                            at += (uint32_t)__popcll(bal);
                        }
                    }
                    next_cnt += total;
                    __syncthreads();                             // w_tile is reused by the next tile
                }
                lev0 = next0;
                cnt = next_cnt;
                ++depth;
            }
        }
    }
    if (tid == 0) {
        b.status[c] = status;
        b.path_len[c] = path_len;
        b.goal_node[c] = goal_node;
        b.n_start[c] = status == OXHIP_ERR_INVALID_START_STATE ? 0u : n_start;
        b.n_goal[c] = status == OXHIP_ERR_INVALID_START_STATE ? 0u : n_goal;
    }
}

// ------------------------------------------------------------------------------------------------
// 3. paths (prm.rs:189-208): [start] ++ (start connection ... goal milestone)

__global__ __launch_bounds__(64) void prm_batch_paths_kernel(PrmBatchArgs b, const uint64_t* __restrict__ row_off, uint32_t* __restrict__ nodes,
                                                              uint64_t* __restrict__ rows) {
    const uint32_t c = blockIdx.x, lane = threadIdx.x, dim = b.dim;
    const uint32_t len = b.path_len[c];
    if (len == 0) return;
    const uint64_t off = row_off[c];                             // relative to the round's first row
    const uint32_t* parent = b.parent + (size_t)c * b.stride;
    const uint64_t* ms = (const uint64_t*)b.ms;                  // rows are copied as words: bit for bit
    const uint64_t* start = (const uint64_t*)b.starts + ((size_t)b.q0 + c) * dim;
    if (lane == 0) nodes[off] = 0xFFFFFFFFu;
    if (lane < dim) rows[off * dim + lane] = start[lane];
    uint32_t v = (uint32_t)b.goal_node[c];
    for (uint32_t j = len - 1u; j >= 1u; --j) {                  // every lane walks the chain; lane j % 64 writes row j
        if ((j & 63u) == lane) {
            nodes[off + j] = v;
            for (uint32_t k = 0; k < dim; ++k) rows[(off + j) * dim + k] = ms[(size_t)v * dim + k];
        }
        v = ld_l2(parent + v);
    }
}

// ------------------------------------------------------------------------------------------------
// launchers

void launch_prm_batch_flags(bool so3, const DevParams& p, const PrmBatchArgs& b, double near, hipStream_t s) {
    const dim3 grid(b.n ? (b.n + 255) / 256 : 1, b.n_chunk);
    space_dispatch(prm_space(so3), p.dim, [&](auto d) {
        constexpr int D = decltype(d)::value;
        hipLaunchKernelGGL(prm_batch_flags_kernel<D>, grid, dim3(256), 0, s, SeqSpace<D>::checker(p), b, near);
    });
}

uint32_t prm_batch_group(uint32_t n, uint64_t n_edge_entries) {
    const uint64_t mean = n ? (n_edge_entries + n - 1) / n : 0;
    uint32_t g = 4;
    while (g < 64 && g < mean) g <<= 1;
    return g;
}

constexpr uint32_t kLdsVisitedMax = 1u << 18;   // milestones whose visited bits fit 32 KB of LDS; larger roadmaps go without

template <int G>
static void launch_search(const PrmBatchArgs& b, hipStream_t s) {
    if (b.n <= kLdsVisitedMax)
        hipLaunchKernelGGL((prm_batch_search_kernel<G, true>), dim3(b.n_chunk), dim3(kSearchThreads), ((b.n + 31u) / 32u) * sizeof(uint32_t), s, b);
    else
        hipLaunchKernelGGL((prm_batch_search_kernel<G, false>), dim3(b.n_chunk), dim3(kSearchThreads), 0, s, b);
}

void launch_prm_batch_search(const PrmBatchArgs& b, uint32_t group, hipStream_t s) {
    switch (group) {
        case 4: launch_search<4>(b, s); break;
        case 8: launch_search<8>(b, s); break;
        case 16: launch_search<16>(b, s); break;
        case 32: launch_search<32>(b, s); break;
        default: launch_search<64>(b, s); break;
    }
}

void launch_prm_batch_paths(const PrmBatchArgs& b, const uint64_t* row_off, uint32_t* nodes, double* rows, hipStream_t s) {
    hipLaunchKernelGGL(prm_batch_paths_kernel, dim3(b.n_chunk), dim3(64), 0, s, b, row_off, nodes, (uint64_t*)rows);
}

}  // namespace oxhip
