// shortcut_core.hip -- the shortcut of a round of paths on gfx950 (wave64): the pair matrix and the shortest chain over it, once for
// both entries.  DESIGN.md sections 18 (an RRT batch's extracted paths, m = 1) and 25 (a PRM batch's answered paths, every edge in
// m parts).  A path of L original states is M = (L - 1) m + 1 rows q_0 .. q_{M-1}, q_{k m} = p_k; the window is W = span * m rows.
//
//   1. shortcut_pairs_kernel<D, SUBDIVIDED>   the hot path: one wave per word of the bit matrix, one thread per slot (d - 2) * M + u,
//        2 <= d <= W: check_motion(from = q_u, to = q_{u + d}) by SeqSpace<D>::motion_valid, the ballot is the word (a path's slots
//        are padded to whole words; slots with u + d >= M are idle).  d-major, so the 64 lanes of a wave hold motions of equal index
//        distance -- similar lengths, similar step counts.  A slot whose two rows lie on one original edge is idle: the planner
//        accepted that motion, and this is a part of it.  The midpoint filter runs over a wave-uniform sphere index (scalar loads);
//        its absolute margin is per motion, since a state may lie outside the bounds (the goal centre, a tree given through
//        set_tree).  SUBDIVIDED = false is m = 1 at compile time (no row shares an edge with another but its neighbour): what an
//        RRT batch launches, R^2 .. R^8, SO(3), SO(2).  SUBDIVIDED = true reads m: what a PRM batch launches, R^1 .. R^8, SO(3).
//   2. shortcut_dp_kernel<D>   one wave per path, v serial: cost[v] = min over u in [v - W, v - 1] with valid(u, v) of
//        fl(cost[u] + distance(q_u, q_v)), lowest u among ties (every lane scans its u ascending with strict '<', then the
//        lexicographic (cost, u) minimum over the wave).  Distances are computed on the fly in the space's own evaluation order,
//        unfused.  Then the parent chain from M - 1 is written out in path order.
// D = 1 .. 8 is R^D, D = 0 is SO(3), D = -1 is SO(2) (seq_space.hpp).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "oxhip_host.hpp"
#include "oxhip_internal.hpp"
#include "rrt_device.hpp"
#include "seq_space.hpp"

namespace oxhip {

namespace {

// the entry c of the ascending table t[0 .. n] with t[c] <= x < t[c + 1], for a wave-uniform x (equal neighbours: paths without words)
__device__ __forceinline__ uint32_t uniform_find(const uint64_t* __restrict__ t, uint32_t n, uint64_t x) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = uni((lo + hi) >> 1);
        if (uni64(t[mid]) <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// what one lane stores and another loads: the fences keep the compiler from moving either, the memory is the wave's own
__device__ __forceinline__ void wave_publish() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// 1. the pair matrix

template <int D, bool SUBDIVIDED>
__global__ __launch_bounds__(256) void shortcut_pairs_kernel(typename SeqSpace<D>::Checker p, ShortcutArgs a) {
    using Space = SeqSpace<D>;
    const uint64_t gw = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (gw >= a.n_words) return;                                 // wave-uniform
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t c = uniform_find(a.woff, a.n_chunk, gw);
    const uint32_t m = SUBDIVIDED ? a.m : 1u;
    const ShortcutShape sh = shortcut_shape(uni(a.len[c]), m, a.max_span);   // (a path with words has L >= 2)
    const uint32_t M = (uint32_t)sh.rows;
    const uint64_t slot = (gw - uni64(a.woff[c])) * 64u + lane;
    const uint64_t dd = slot / M;                                // d - 2
    const uint32_t u = (uint32_t)(slot - dd * M);
    bool active = dd + 2u <= sh.window && (uint64_t)u + dd + 2u < M;
    if (SUBDIVIDED && active) active = u / m != (u + (uint32_t)dd + 1u) / m;   // both on one original edge: valid without a check
    const uint64_t row_u = uni64(a.row_off[c]) + u;              // rows of `rows`, not of the path: one base pointer stays live
    const uint64_t row_v = row_u + (active ? dd + 2u : 0u);
    bool ok = false;
    if (active) {
        double from[Space::W], to[Space::W];
        Space::load(a.rows + row_u * Space::W, from);
        Space::load(a.rows + row_v * Space::W, to);
        ok = Space::motion_valid(p, from, to, Space::motion_margin(a.filt_base, from, to));
    }
    const uint64_t word = __ballot(ok);
    if (lane == 0) a.bits[gw] = word;
}

// ------------------------------------------------------------------------------------------------
// 2. the shortest chain over the valid pairs

template <int D>
__global__ __launch_bounds__(64) void shortcut_dp_kernel(ShortcutArgs a, ShortcutOut o) {
    using Space = SeqSpace<D>;
    constexpr int W = Space::W;
    const uint32_t c = blockIdx.x, lane = threadIdx.x;
    const uint32_t L = a.len[c];
    if (L == 0) {
        if (lane == 0) { o.simp_len[c] = 0; o.raw_cost[c] = 0.0; o.simp_cost[c] = 0.0; o.checks[c] = 0; }
        return;
    }
    const uint32_t m = a.m;
    const ShortcutShape sh = shortcut_shape(L, m, a.max_span);
    const uint32_t M = (uint32_t)sh.rows, Wd = (uint32_t)sh.window;
    const uint64_t base = a.row_off[c];
    const double* rows = a.rows + base * W;
    const uint64_t* bits = a.bits + a.woff[c];
    double* cost = o.cost + base;
    uint32_t* par = o.par + base;
    uint32_t* idx = o.idx + base;
    if (lane == 0) { cost[0] = 0.0; par[0] = 0u; }
    wave_publish();
    double raw = 0.0;
    uint32_t edge0 = 0;                                          // first row of the original edge that v - 1 lies on
    for (uint32_t v = 1; v < M; ++v) {
        if (v - 1u == edge0 + m) edge0 += m;
        double qv[W];
        Space::load(rows + (uint64_t)v * W, qv);
        Exact best{__builtin_inf(), 0xFFFFFFFFu};
        for (uint32_t u = (v > Wd ? v - Wd : 0u) + lane; u < v; u += 64u) {
            bool ok = u >= edge0;                                // both on one original edge: the planner accepted it
            if (!ok) {
                const uint64_t slot = (uint64_t)(v - u - 2u) * M + u;
                ok = (bits[slot >> 6] >> (slot & 63u)) & 1ull;
            }
            if (ok) {
                double qu[W];
                Space::load(rows + (uint64_t)u * W, qu);
                const double cand = cost[u] + Space::distance(qu, qv);
                if (cand < best.dist) { best.dist = cand; best.idx = u; }
            }
        }
        const Exact r = exact_wave_reduce(best);
        if (v == edge0 + m) {                                    // an original edge ends at v: p_k -> p_{k+1}
            double q0[W];
            Space::load(rows + (uint64_t)edge0 * W, q0);
            raw = raw + Space::distance(q0, qv);
        }
        if (lane == 0) { cost[v] = r.dist; par[v] = r.idx < v ? r.idx : v - 1u; }
        wave_publish();
    }
    // the parent chain from M - 1, in path order
    uint32_t n = 1;
    for (uint32_t v = M - 1u; v != 0u; v = par[v]) ++n;
    uint32_t v = M - 1u;
    for (uint32_t t = n; t-- > 0;) {
        if ((t & 63u) == lane) idx[t] = v;
        v = par[v];
    }
    if (lane == 0) {
        o.simp_len[c] = n;
        o.raw_cost[c] = raw;
        o.simp_cost[c] = cost[M - 1u];
        o.checks[c] = sh.checks;
    }
}

// ------------------------------------------------------------------------------------------------
// launchers

void launch_shortcut_pairs(const DevParams& p, const ShortcutArgs& a, bool subdivided, hipStream_t s) {
    if (a.n_words == 0) return;
    const dim3 grid((uint32_t)((a.n_words + 3u) / 4u)), block(256);
    if (subdivided)
        space_dispatch(p.space, p.dim, [&](auto d) {
            constexpr int D = decltype(d)::value;
            hipLaunchKernelGGL((shortcut_pairs_kernel<D, true>), grid, block, 0, s, SeqSpace<D>::checker(p), a);
        });
    else
        space_dispatch<2, true>(p.space, p.dim, [&](auto d) {   // (an R^n batch has at least two dimensions here: simplify_supported)
            constexpr int D = decltype(d)::value;
            hipLaunchKernelGGL((shortcut_pairs_kernel<D, false>), grid, block, 0, s, SeqSpace<D>::checker(p), a);
        });
}

void launch_shortcut_dp(uint32_t space, uint32_t dim, const ShortcutArgs& a, const ShortcutOut& o, hipStream_t s) {
    space_dispatch<1, true>(space, dim, [&](auto d) {
        constexpr int D = decltype(d)::value;
        hipLaunchKernelGGL(shortcut_dp_kernel<D>, dim3(a.n_chunk), dim3(64), 0, s, a, o);
    });
}

}  // namespace oxhip
