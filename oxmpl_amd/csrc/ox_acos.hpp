// ox_acos.hpp -- arc cosine of the SO(3) space (oxmpl/src/base/spaces/so3_state_space.rs:101-110 and :137-139 call
// abs_dot.acos() / dot.acos(), i.e. whatever libm the host has).  One portable routine instead: the acos of FreeBSD msun
// (e_acos.c: a rational approximation of asin on [0, 0.5] and the half-angle identities above it), every operation a
// single unfused binary64 operation (the translation unit is built with -ffp-contract=off), so the device and the CPU
// checker of the test suite, which restates it operation for operation, agree bit for bit.  Below one ulp; against a
// given libm the last bit differs now and then.  NaN for |x| > 1 and for NaN.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace oxhip {

__device__ __forceinline__ double ox_acos_r(double z) {   // R(z) = P(z) / Q(z), asin(x) ~ x + x R(x^2)
    const double pS0 = 1.66666666666666657415e-01, pS1 = -3.25565818622400915405e-01, pS2 = 2.01212532134862925881e-01,
                 pS3 = -4.00555345006794114027e-02, pS4 = 7.91534994289814532176e-04, pS5 = 3.47933107596021167570e-05,
                 qS1 = -2.40339491173441421878e+00, qS2 = 2.02094576023350569471e+00, qS3 = -6.88283971605453293030e-01,
                 qS4 = 7.70381505559019352791e-02;
    const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
    const double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
    return p / q;
}

__device__ __forceinline__ double ox_acos(double x) {
    const double pi = 3.14159265358979311600e+00, pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17;
    const int32_t hx = __double2hiint(x);
    const uint32_t ix = (uint32_t)hx & 0x7fffffffu;
    if (ix >= 0x3ff00000u) {   // |x| >= 1 (or NaN)
        if (ix == 0x3ff00000u && __double2loint(x) == 0) return hx > 0 ? 0.0 : pi + 2.0 * pio2_lo;
        return __builtin_nan("");
    }
    if (ix < 0x3fe00000u) {   // |x| < 0.5
        if (ix <= 0x3c600000u) return pio2_hi + pio2_lo;
        const double z = x * x;
        const double r = ox_acos_r(z);
        return pio2_hi - (x - (pio2_lo - x * r));
    }
    if (hx < 0) {   // x <= -0.5
        const double z = (1.0 + x) * 0.5;
        const double s = sqrt(z);
        const double r = ox_acos_r(z);
        const double w = r * s - pio2_lo;
        return pi - 2.0 * (s + w);
    }
    // x >= 0.5: 2 asin(sqrt((1 - x) / 2)), the square root split into a 32-bit head df and a correction c
    const double z = (1.0 - x) * 0.5;
    const double s = sqrt(z);
    const double df = __hiloint2double(__double2hiint(s), 0);
    const double c = (z - df * df) / (s + df);
    const double r = ox_acos_r(z);
    const double w = r * s + c;
    return 2.0 * (df + w);
}

}  // namespace oxhip
