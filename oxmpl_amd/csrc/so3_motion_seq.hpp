// so3_motion_seq.hpp -- SO(3) check_motion evaluated by ONE thread, and the slice of DevParams the PRM kernels over SO(3) read:
// shared by prm_so3.hip (edge and query kernels) and prm_batch.hip (the batched query's flag kernel).
#pragma once
#include "rrt_device.hpp"
#include "so3_device.hpp"

namespace oxhip {

struct So3Cones {           // what the edge and query kernels read of DevParams (the whole struct costs SGPRs)
    const double* c;        // centres SoA [4][n]
    const double* r;        // radii [n]
    uint32_t n;
    double res;             // check_motion's step length
};

// check_motion (prm.rs:161-187, the discretisation of rrt.rs:90-116) by one thread; is_valid is pure, so stopping at the first
// invalid state is the reference's early return
__device__ __forceinline__ bool so3_motion_valid_seq(const double* cc, uint32_t stride, const double* cr, uint32_t nc, const double from[4],
                                                     const double to[4], double res) {
    if (nc == 0) return true;
    const uint32_t nsteps = num_steps_u32(so3_distance(from, to), res);
    if (nsteps <= 1u) return !so3_cone_hit(cc, stride, cr, nc, to);
    const double dn = (double)nsteps;
    for (uint32_t s = 1; s <= nsteps; ++s) {   // nsteps <= 0.5 PI / res <= 1e6 (checked at create)
        double st[4];
        so3_interpolate(from, to, (double)s / dn, st);
        if (so3_cone_hit(cc, stride, cr, nc, st)) return false;
    }
    return true;
}

}  // namespace oxhip
