// prm_path_simplify.hip -- the answered paths of a PRM batch, subdivided and shortcut on gfx950 (wave64).  DESIGN.md section 25;
// include/oxmpl_hip.h states the semantics (oxhip_prm_batch_simplify_paths).
//
//   1. dense_rows_kernel<D>   one thread per row of the dense path: q_{k m} is p_k copied as 64-bit words, q_{k m + r} is the
//        space's own interpolate(p_k, p_{k+1}, (double)r / (double)m), unfused (lerp / so3_interpolate: the bits of
//        oxhip_interpolate_batch and of the interpolate op of oxhip_so3_op_batch).
//   2. dense_pairs_kernel<D>  the hot path, path_pairs_kernel's shape over the dense path: one wave per word of the bit matrix,
//        one thread per slot (d - 2) * M + u, check_motion(from = q_u, to = q_{u + d}) by SeqSpace<D>::motion_valid with the
//        per-motion margin, the ballot is the word.  A slot whose two points lie on one original edge is idle: the roadmap
//        accepted that motion, and this is a part of it.  d-major, so a wave's lanes hold motions of similar length.
//   3. dense_dp_kernel<D>     one wave per query, v serial: cost[v] = min over u in [v - W, v - 1] with valid(u, v) of
//        fl(cost[u] + distance(q_u, q_v)), lowest u among ties (every lane scans its u ascending with strict '<', then the
//        lexicographic (cost, u) minimum over the wave); then the parent chain from M - 1 in path order.
//   4. dense_gather_kernel    the chain's indices and rows, compacted behind the query's offset for one copy to the host.
// D = 1 .. 8 is R^D, D = 0 is SO(3) (seq_space.hpp); nothing is instantiated over SO(2): no roadmap is built there.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "oxhip_internal.hpp"
#include "rrt_device.hpp"
#include "seq_space.hpp"

namespace oxhip {

namespace {

// the space's own interpolation between two states
template <int D>
__device__ __forceinline__ void dense_interpolate(const double* from, const double* to, double t, double* out) {
    if constexpr (D == 0) so3_interpolate(from, to, t, out);
    else lerp<D>(from, to, t, out, D);
}

__device__ __forceinline__ uint32_t dense_span(uint32_t L, uint32_t max_span) {   // in original edges
    const uint32_t full = L - 1u;
    return max_span == 0u || max_span > full ? full : max_span;
}

// the entry c of the ascending table t[0 .. n] with t[c] <= x < t[c + 1] (equal neighbours: queries without rows / words)
__device__ __forceinline__ uint32_t dense_find(const uint64_t* __restrict__ t, uint32_t n, uint64_t x) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (t[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// 1. the dense path

template <int D>
__global__ __launch_bounds__(256) void dense_rows_kernel(DenseArgs a) {
    using Space = SeqSpace<D>;
    constexpr int W = Space::W;
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (g >= a.n_rows) return;
    const uint32_t c = dense_find(a.doff, a.n_chunk, g);
    const uint32_t u = (uint32_t)(g - a.doff[c]);
    const uint32_t k = u / a.m, r = u - k * a.m;
    const uint64_t raw = a.off[a.q0 + c] + k;
    if (r == 0u) {
        const uint64_t* src = (const uint64_t*)a.rows + raw * W;
        uint64_t* dst = (uint64_t*)a.dense + g * W;
#pragma unroll
        for (int j = 0; j < W; ++j) dst[j] = src[j];
        return;
    }
    double from[W], to[W], out[W];
    Space::load(a.rows + raw * W, from);
    Space::load(a.rows + (raw + 1u) * W, to);
    const double t = (double)r / (double)a.m;
    dense_interpolate<D>(from, to, t, out);
#pragma unroll
    for (int j = 0; j < W; ++j) a.dense[g * W + j] = out[j];
}

// ------------------------------------------------------------------------------------------------
// 2. the pair matrix

template <int D>
__global__ __launch_bounds__(256) void dense_pairs_kernel(typename SeqSpace<D>::Checker p, DenseArgs a) {
    using Space = SeqSpace<D>;
    const uint64_t gw = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (gw >= a.n_words) return;                                 // wave-uniform
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t lo = 0, hi = a.n_chunk;                             // woff[lo] <= gw < woff[hi], wave-uniform
    while (hi - lo > 1u) {
        const uint32_t mid = uni((lo + hi) >> 1);
        if (uni64(a.woff[mid]) <= gw) lo = mid; else hi = mid;
    }
    const uint32_t c = lo;
    const uint32_t L = uni(a.len[a.q0 + c]);
    const uint32_t M = (L - 1u) * a.m + 1u;
    const uint32_t Wd = dense_span(L, a.max_span) * a.m;
    const uint64_t slot = (gw - uni64(a.woff[c])) * 64u + lane;
    const uint64_t dd = slot / M;                                // d - 2
    const uint32_t u = (uint32_t)(slot - dd * M);
    bool active = dd + 2u <= Wd && (uint64_t)u + dd + 2u < M;
    const uint32_t v = active ? u + (uint32_t)dd + 2u : u;
    if (active) active = u / a.m != (v - 1u) / a.m;              // both on one original edge: valid without a check
    bool ok = false;
    if (active) {
        const double* rows = a.dense + uni64(a.doff[c]) * Space::W;
        double from[Space::W], to[Space::W];
        Space::load(rows + (uint64_t)u * Space::W, from);
        Space::load(rows + (uint64_t)v * Space::W, to);
        ok = Space::motion_valid(p, from, to, Space::motion_margin(a.filt_base, from, to));
    }
    const uint64_t word = __ballot(ok);
    if (lane == 0) a.bits[gw] = word;
}

// ------------------------------------------------------------------------------------------------
// 3. the shortest chain over the valid pairs

namespace {
// what one lane stores and another loads: the fences keep the compiler from moving either, the memory is the wave's own
__device__ __forceinline__ void dense_publish() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
}  // namespace

template <int D>
__global__ __launch_bounds__(64) void dense_dp_kernel(DenseArgs a, DenseOut o) {
    using Space = SeqSpace<D>;
    constexpr int W = Space::W;
    const uint32_t c = blockIdx.x, lane = threadIdx.x;
    const uint32_t L = a.len[a.q0 + c];
    if (L == 0) {
        if (lane == 0) { o.simp_len[c] = 0; o.raw_cost[c] = 0.0; o.simp_cost[c] = 0.0; o.checks[c] = 0; }
        return;
    }
    const uint32_t m = a.m;
    const uint32_t M = (L - 1u) * m + 1u;
    const uint32_t Wd = dense_span(L, a.max_span) * m;
    const uint64_t base = a.doff[c];
    const double* rows = a.dense + base * W;
    const uint64_t* bits = a.bits + a.woff[c];
    double* cost = o.cost + base;
    uint32_t* par = o.par + base;
    uint32_t* idx = o.idx + base;
    if (lane == 0) { cost[0] = 0.0; par[0] = 0u; }
    dense_publish();
    double raw = 0.0;
    uint32_t edge0 = 0;                                          // first dense index of the original edge that v - 1 lies on
    for (uint32_t v = 1; v < M; ++v) {
        if (v - 1u == edge0 + m) edge0 += m;
        double qv[W];
        Space::load(rows + (uint64_t)v * W, qv);
        Exact best{__builtin_inf(), 0xFFFFFFFFu};
        for (uint32_t u = (v > Wd ? v - Wd : 0u) + lane; u < v; u += 64u) {
            bool ok = u >= edge0;                                // both on one original edge
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
        dense_publish();
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
        // pairs with 1 <= d <= Wd: sum of (M - d); of them on one edge: m (m + 1) / 2 per original edge
        o.checks[c] = (uint64_t)Wd * M - (uint64_t)Wd * (Wd + 1ull) / 2ull - (uint64_t)(L - 1u) * ((uint64_t)m * (m + 1ull) / 2ull);
    }
}

// ------------------------------------------------------------------------------------------------
// 4. the chains, compacted

__global__ __launch_bounds__(64) void dense_gather_kernel(DenseArgs a, DenseOut o, uint32_t width) {
    const uint32_t c = blockIdx.x, lane = threadIdx.x;
    const uint32_t n = o.simp_len[c];
    const uint64_t base = a.doff[c], out = o.soff[c];
    const uint64_t* rows = (const uint64_t*)a.dense + base * width;
    uint64_t* dst = (uint64_t*)o.out_rows;
    for (uint32_t t = lane; t < n; t += 64u) {
        const uint32_t u = o.idx[base + t];
        o.out_idx[out + t] = u;
        for (uint32_t j = 0; j < width; ++j) dst[(out + t) * width + j] = rows[(uint64_t)u * width + j];
    }
}

// ------------------------------------------------------------------------------------------------
// launchers

uint64_t dense_path_rows(uint32_t L, uint32_t m) { return L ? (uint64_t)(L - 1u) * m + 1u : 0u; }

uint64_t dense_pair_words(uint32_t L, uint32_t m, uint32_t max_span) {
    if (L < 2) return 0;
    const uint32_t full = L - 1u;
    const uint64_t S = max_span == 0u || max_span > full ? full : max_span;
    const uint64_t Wd = S * m;
    if (Wd < 2) return 0;
    return ((Wd - 1u) * dense_path_rows(L, m) + 63u) / 64u;
}

void launch_dense_rows(bool so3, uint32_t dim, const DenseArgs& a, hipStream_t s) {
    if (a.n_rows == 0) return;
    const dim3 grid((uint32_t)((a.n_rows + 255u) / 256u)), block(256);
    space_dispatch(prm_space(so3), dim, [&](auto d) {
        constexpr int D = decltype(d)::value;
        hipLaunchKernelGGL(dense_rows_kernel<D>, grid, block, 0, s, a);
    });
}

void launch_dense_pairs(const DevParams& p, const DenseArgs& a, hipStream_t s) {
    if (a.n_words == 0) return;
    const dim3 grid((uint32_t)((a.n_words + 3u) / 4u)), block(256);
    space_dispatch(p.space, p.dim, [&](auto d) {
        constexpr int D = decltype(d)::value;
        hipLaunchKernelGGL(dense_pairs_kernel<D>, grid, block, 0, s, SeqSpace<D>::checker(p), a);
    });
}

void launch_dense_dp(bool so3, uint32_t dim, const DenseArgs& a, const DenseOut& o, hipStream_t s) {
    space_dispatch(prm_space(so3), dim, [&](auto d) {
        constexpr int D = decltype(d)::value;
        hipLaunchKernelGGL(dense_dp_kernel<D>, dim3(a.n_chunk), dim3(64), 0, s, a, o);
    });
}

void launch_dense_gather(uint32_t width, const DenseArgs& a, const DenseOut& o, hipStream_t s) {
    hipLaunchKernelGGL(dense_gather_kernel, dim3(a.n_chunk), dim3(64), 0, s, a, o, width);
}

}  // namespace oxhip
