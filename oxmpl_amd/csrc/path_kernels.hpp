// path_kernels.hpp -- the shortcutter's pair-matrix and DP kernels (path_simplify.hip's header describes them), written once over
// SeqSpace<D> / the space kind.  path_simplify.hip instantiates them for R^n and SO(3); rrt_so2_services.hip for SO(2).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "oxhip_internal.hpp"
#include "rrt_device.hpp"
#include "seq_space.hpp"

namespace oxhip {

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

}  // namespace oxhip
