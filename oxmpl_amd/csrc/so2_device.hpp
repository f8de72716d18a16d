// so2_device.hpp -- SO2StateSpace arithmetic (oxmpl/src/base/spaces/so2_state_space.rs, oxmpl/src/base/states/so2_state.rs) in
// unfused binary64, in the reference's order, and the forbidden-arc checker of the reference's SO(2) fixture
// (oxmpl/tests/rrt_so2ss_tests.rs, ForbiddenAngleChecker).  Shared by rrt_connect_se2.hip (the heading of an SE(2) state),
// rrt_so2.hip (RRT over SO(2)) and seq_space.hpp (the one-thread view of the space).
#pragma once
#include "rrt_device.hpp"

namespace oxhip {

#define OXHIP_PI 3.14159265358979323846   // std::f64::consts::PI = 0x400921FB54442D18

// f64::rem_euclid(a, 2*PI): r = a % (2*PI); if r < 0.0 { r + 2*PI } else { r }.  fmod is exact, and for
// -2*PI < a < 4*PI it needs no division: a in [2*PI, 4*PI) gives a - 2*PI (exact by Sterbenz' lemma, which is
// fmod's value), a in [0, 2*PI) gives a, a in (-2*PI, 0) gives a, to which the reference then adds 2*PI -- the
// same rounded addition.  Everything a planner run produces lies in that window; the rest takes fmod.
__device__ __forceinline__ double rem_euclid_2pi(double a) {
    const double b = 2.0 * OXHIP_PI;
    // the window, by selects (one uniform branch instead of a chain of divergent ones: this runs several times per extend)
    double r = a;                                  // a in [0, b), a in (-b, 0), -0.0: fmod's value is a itself
    r = (a >= b) ? a - b : r;                      // a in [b, 2 b): fmod's value, exactly (Sterbenz)
    if (__builtin_expect(__ballot(!(a > -b && a < 2.0 * b)) != 0, 0)) {   // outside the window (or NaN): fmod proper
        if (!(a > -b && a < 2.0 * b)) r = fmod(a, b);
    }
    return r < 0.0 ? r + b : r;
}
__device__ __forceinline__ double so2_normalise(double v) { return rem_euclid_2pi(v + OXHIP_PI) - OXHIP_PI; }
__device__ __forceinline__ double so2_distance(double a, double b) {
    double diff = a - b;
    diff = rem_euclid_2pi(diff + OXHIP_PI) - OXHIP_PI;
    return fabs(diff);
}
__device__ __forceinline__ double so2_interpolate(double from, double to, double t) {
    double d = so2_normalise(to) - so2_normalise(from);
    if (d > OXHIP_PI) d -= 2.0 * OXHIP_PI;
    else if (d < -OXHIP_PI) d += 2.0 * OXHIP_PI;
    const double out = from + d * t;
    return so2_normalise(out);
}

// ForbiddenAngleChecker::is_valid, negated, over n arcs: !(min <= normalise(v) <= max) for every arc, closed on both ends.  A NaN
// (state or arc end) fails both comparisons: no hit.
__device__ __forceinline__ bool so2_arc_hit(const double* lo, const double* hi, uint32_t n, double v) {
    const double nv = so2_normalise(v);
    bool hit = false;
    for (uint32_t j = 0; j < n; ++j) hit = hit || (lo[j] <= nv && nv <= hi[j]);
    return hit;
}

struct So2Arcs {            // what the one-thread kernels read of DevParams
    const double* lo;       // arc minima [n]  (DevParams::box_lo, 1-wide rows)
    const double* hi;       // arc maxima [n]
    uint32_t n;
    double res;             // check_motion's step length
};

// check_motion (rrt.rs:90-116) by one thread; is_valid is pure, so stopping at the first invalid state is the reference's early return
__device__ __forceinline__ bool so2_motion_valid_seq(const double* lo, const double* hi, uint32_t n, double from, double to, double res) {
    if (n == 0) return true;
    const uint32_t nsteps = num_steps_u32(so2_distance(from, to), res);
    if (nsteps <= 1u) return !so2_arc_hit(lo, hi, n, to);
    const double dn = (double)nsteps;
    for (uint32_t s = 1; s <= nsteps; ++s) {   // nsteps <= PI / res <= 1e6 (checked at create)
        if (so2_arc_hit(lo, hi, n, so2_interpolate(from, to, (double)s / dn))) return false;
    }
    return true;
}

}  // namespace oxhip
