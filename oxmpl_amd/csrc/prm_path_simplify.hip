// prm_path_simplify.hip -- the answered paths of a PRM batch, subdivided for the shortcut and compacted after it, on gfx950
// (wave64).  DESIGN.md section 25; include/oxmpl_hip.h states the semantics (oxhip_prm_batch_simplify_paths).  The pair matrix
// and the shortest chain over the dense rows are shortcut_core.hip's.
//
//   1. dense_rows_kernel<D>   one thread per row of the dense path: q_{k m} is p_k copied as 64-bit words, q_{k m + r} is the
//        space's own interpolate(p_k, p_{k+1}, (double)r / (double)m), unfused (lerp / so3_interpolate: the bits of
//        oxhip_interpolate_batch and of the interpolate op of oxhip_so3_op_batch).
//   2. dense_gather_kernel    the chain's indices and rows, compacted behind the query's offset for one copy to the host.
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
// 2. the chains, compacted

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

void launch_dense_rows(bool so3, uint32_t dim, const DenseArgs& a, hipStream_t s) {
    if (a.n_rows == 0) return;
    const dim3 grid((uint32_t)((a.n_rows + 255u) / 256u)), block(256);
    space_dispatch(prm_space(so3), dim, [&](auto d) {
        constexpr int D = decltype(d)::value;
        hipLaunchKernelGGL(dense_rows_kernel<D>, grid, block, 0, s, a);
    });
}

void launch_dense_gather(uint32_t width, const DenseArgs& a, const DenseOut& o, hipStream_t s) {
    hipLaunchKernelGGL(dense_gather_kernel, dim3(a.n_chunk), dim3(64), 0, s, a, o, width);
}

}  // namespace oxhip
