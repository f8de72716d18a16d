// so3_device.hpp -- SO(3) arithmetic of the device path: SO3StateSpace (oxmpl/src/base/spaces/so3_state_space.rs) restated
// in unfused binary64 in the reference's evaluation order (the translation units are built with -ffp-contract=off).
// States are unit quaternions (x, y, z, w) (states/so3_state.rs:13-19); normalising the inputs is the caller's job, as in
// the reference.  acos is ox_acos and sin is ox_sincos (portable routines the CPU checker restates operation for operation),
// so against a rustc-built oxmpl (libm) an evaluation is within a few ulp, not bit-exact: PARITY UNPINNED.
//
//   distance      so3_state_space.rs:101-110   abs_dot > 1 - 1e-9 ? 0 : acos(abs_dot)
//   interpolate   so3_state_space.rs:117-159   LERP + normalise when dot > 0.9995 (after the sign flip), else SLERP
//   validity      oxmpl/tests/rrt_so3ss_tests.rs:46-56   ForbiddenConeChecker: distance(centre, q) > radius
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ox_acos.hpp"
#include "ox_sincos.hpp"

namespace oxhip {

__device__ __forceinline__ double so3_dot(const double a[4], const double b[4]) {
    const double p0 = a[0] * b[0], p1 = a[1] * b[1], p2 = a[2] * b[2], p3 = a[3] * b[3];
    double s = p0 + p1;
    s = s + p2;
    return s + p3;
}

__device__ __forceinline__ double so3_distance(const double a[4], const double b[4]) {
    const double abs_dot = fabs(so3_dot(a, b));
    return abs_dot > 1.0 - 1e-9 ? 0.0 : ox_acos(abs_dot);
}

__device__ __forceinline__ void so3_interpolate(const double from[4], const double to[4], double t, double out[4]) {
    double dot = so3_dot(from, to);
    const double sign = dot < 0.0 ? -1.0 : 1.0;
    dot = dot * sign;
    if (dot > 0.9995) {   // LERP: from + t * (to * sign - from), then divide by the norm (powi(2) is x * x)
        double o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double ts = to[k] * sign;
            const double d = ts - from[k];
            const double sc = t * d;
            o[k] = from[k] + sc;
        }
        const double q0 = o[0] * o[0], q1 = o[1] * o[1], q2 = o[2] * o[2], q3 = o[3] * o[3];
        double ns = q0 + q1;
        ns = ns + q2;
        ns = ns + q3;
        const double norm = sqrt(ns);
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k] = o[k] / norm;
        return;
    }
    // SLERP: theta = acos(dot); s0 = sin((1 - t) theta) / sin(theta); s1 = sin(t theta) / sin(theta) * sign
    const double theta = ox_acos(dot);
    double sin_theta, c_unused, sa, sb;
    ox_sincos(theta, sin_theta, c_unused);
    const double a = (1.0 - t) * theta;
    const double b = t * theta;
    ox_sincos(a, sa, c_unused);
    ox_sincos(b, sb, c_unused);
    const double s0 = sa / sin_theta;
    double s1 = sb / sin_theta;
    s1 = s1 * sign;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double u = from[k] * s0, v = to[k] * s1;
        out[k] = u + v;
    }
}

// rand 0.9 random_range(-1.0..1.0) from one word: (bits >> 12 | 1.0) - 1.0, times scale 2.0, plus -1.0; false when rand would
// draw again (res >= 1.0: not reachable for this range -- the largest value is 1 - 2^-51 -- but stated as rand states it)
__device__ __forceinline__ bool so3_range_word(uint64_t w, double& res) {
    const double v01 = __longlong_as_double((long long)((w >> 12) | 0x3FF0000000000000ull)) - 1.0;
    res = v01 * 2.0;
    res = res + -1.0;
    return res < 1.0;
}

// one rejection attempt of so3_state_space.rs:213-229 from its four coordinates; true when accepted (q written)
__device__ __forceinline__ bool so3_attempt(const double v[4], const double centre[4], double max_angle, double q[4]) {
    const double x2 = v[0] * v[0], y2 = v[1] * v[1], z2 = v[2] * v[2], w2 = v[3] * v[3];
    double ns = x2 + y2;
    ns = ns + z2;
    ns = ns + w2;
    if (!(ns > 1e-9 && ns < 1.0)) return false;
    const double norm = sqrt(ns);
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = v[k] / norm;
    return so3_distance(centre, q) <= max_angle;
}

// is state s inside one of the n cones (centres SoA [4][stride], radii r[n])?  valid iff distance(centre, s) > radius (strict)
__device__ __forceinline__ bool so3_cone_hit(const double* cc, uint32_t stride, const double* cr, uint32_t n, const double s[4]) {
    bool hit = false;
    for (uint32_t j = 0; j < n; ++j) {
        const double c[4] = {cc[j], cc[stride + j], cc[2 * stride + j], cc[3 * stride + j]};
        hit = hit || !(so3_distance(c, s) > cr[j]);
    }
    return hit;
}

}  // namespace oxhip
