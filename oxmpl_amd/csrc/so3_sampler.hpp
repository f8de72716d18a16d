// so3_sampler.hpp -- SO3StateSpace::sample_uniform (oxmpl/src/base/spaces/so3_state_space.rs:201-231) by one wave: the 64 rejection
// attempts of a round are evaluated side by side.  Shared by rrt_so3.hip (RRT over SO(3)) and rrt_connect_se3.hip (the rotation
// part of an SE(3) sample); arithmetic: so3_device.hpp.
#pragma once
#include "rrt_device.hpp"
#include "lane_sampler.hpp"
#include "so3_device.hpp"

namespace oxhip {

// sample_uniform by one lane after the other, word by word (random_range redraws included)
__device__ __forceinline__ void so3_sample_serial(RngWindow& rng, const DevParams& p, double q[4]) {
    for (;;) {
        double v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            while (!so3_range_word(rng.next<false>(), v[k])) {}
        if (so3_attempt(v, p.so3_centre, p.so3_max_angle, q)) return;
    }
}

// sample_uniform for the space (p.so3_centre, p.so3_max_angle).  Wave-uniform result.  Lane j evaluates attempt j of the round (its
// four words follow the 4 j words of the attempts before it); the first accepted attempt wins and the stream moves past it.  A round
// without an accepted attempt moves 256 words on and tries the next 64.  A range redraw at or before the winner (or the test switch
// OXHIP_DEBUG_SO3_SERIAL_SAMPLER) hands the sample to the serial form.
__device__ __forceinline__ void so3_sample_uniform_wave(RngWindow& rng, const DevParams& p, uint32_t lane, double q[4]) {
    if (p.so3_max_angle < 1e-9) {   // the centre of a degenerate space (so3_state_space.rs:204-206): no draw
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = p.so3_centre[k];
        return;
    }
    if (p.dbg_flags & OXHIP_DEBUG_SO3_SERIAL_SAMPLER) { so3_sample_serial(rng, p, q); return; }
    for (;;) {
        const uint64_t pos = rng.pos;
        rng_window_hold(rng, 256, lane);   // the window must hold the round's 256 words
        const uint32_t rel0 = (uint32_t)(pos - rng.base_blk * 8) + 4u * lane;
        double v[4];
        bool redraw = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t a = rel0 + (uint32_t)k, bl = a >> 3, w = (a & 7u) * 2u;
            const uint64_t word = ((uint64_t)rng.buf[w + 1][bl] << 32) | rng.buf[w][bl];
            redraw = redraw || !so3_range_word(word, v[k]);
        }
        double qa[4] = {0.0, 0.0, 0.0, 0.0};
        const bool acc = !redraw && so3_attempt(v, p.so3_centre, p.so3_max_angle, qa);
        const uint64_t am = __ballot(acc), rm = __ballot(redraw);
        const uint32_t L = am ? (uint32_t)__builtin_ctzll(am) : 64u;
        const uint64_t upto = L >= 63u ? ~0ull : (2ull << L) - 1ull;
        if (rm & upto) { so3_sample_serial(rng, p, q); return; }   // (rng.pos is still the round's start)
        if (am == 0) { rng.pos = uni64(pos + 256); continue; }
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = readlane_f64(qa[k], (int)L);
        rng.pos = uni64(pos + 4ull * (L + 1u));
        return;
    }
}

}  // namespace oxhip
