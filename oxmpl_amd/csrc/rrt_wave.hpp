// rrt_wave.hpp -- what the one-wave-per-problem RRT kernels of the rotation spaces (rrt_so2.hip, rrt_so3.hip) share: the fence
// behind which lane 0's store becomes the wave's, and check_motion dealt to the lanes 64 states per pass.  The planner loops
// stay in the two files: written once over an adapter, the loop compiled to a slightly different code object for either space and
// did not hold the hand-written loops' speed (SO(3) 0.15 % slower, SO(2)'s growth scene 0.7 %: DESIGN.md section 22); with these
// two helpers the kernels compile to the instructions they had before.
//
// The motion pass takes the space as a small struct:
//   W                        components of a state
//   distance, interpolate    the space's arithmetic on double[W]
//   free(), state_hit(s)     the checker: no obstacle at all; state s is invalid
#pragma once
#include "rrt_device.hpp"

namespace oxhip {

// what one lane stores and another loads: LDS is in order per wave, the fences keep the compiler from moving either access
__device__ __forceinline__ void rrt_wave_publish() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// check_motion (rrt.rs:90-116) by one wave: lane s tests state s + 1 of the steps 1 ..= nsteps (or `to` alone when nsteps <= 1)
// against every obstacle; returns the wave-uniform verdict "some state is invalid".  is_valid is pure, so testing a whole pass of
// states equals the reference's first-invalid early exit.
template <typename Space>
__device__ __forceinline__ bool rrt_wave_motion_invalid(const Space& sp, const double from[Space::W], const double to[Space::W], double res,
                                                        uint32_t lane) {
    constexpr int W = Space::W;
    if (sp.free()) return false;
    const uint32_t nsteps = num_steps_u32(sp.distance(from, to), res);
    const uint32_t S = nsteps <= 1u ? 1u : nsteps;
    const double dn = (double)nsteps;
    for (uint32_t s0 = 0; s0 < S; s0 += 64u) {
        const uint32_t s = s0 + lane;
        bool bad = false;
        if (s < S) {
            double st[W];
#pragma unroll
            for (int k = 0; k < W; ++k) st[k] = to[k];
            if (nsteps > 1u) sp.interpolate(from, to, (double)(s + 1u) / dn, st);
            bad = sp.state_hit(st);
        }
        if (__ballot(bad) != 0) return true;
        if (s0 + 64u < s0) break;   // (no wrap at 2^32)
    }
    return false;
}

}  // namespace oxhip
