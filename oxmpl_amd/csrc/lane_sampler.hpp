// lane_sampler.hpp -- THE definition of the lane-parallel draw order: one wave samples up to 64 consecutive iterations of one
// problem side by side, word for word as the reference's sequential loop consumes the stream (rrt.rs:177-184 resp.
// rrt_connect.rs:258-262: random_bool(goal_bias), then sample_goal or sample_uniform, real_vector_state_space.rs:233-249).
// Every kernel that samples a block of iterations at once goes through here (rrt_resident.hip, rrt_lanes.hip, rrt_cells.hip,
// rrt_connect.hip, rrt_connect_se2.hip); they differ only in where a sample is stored.  The sequential form is sample_state
// (rrt_device.hpp), which is also the fallback below.
#pragma once

#include "rrt_device.hpp"

namespace oxhip {

// Keeps the next `words` words of the stream inside the wave-private LDS window: when the position has left the window, or the
// words would run past its end, the window restarts at the position's block (64 blocks = 512 words, one block per lane,
// written word-major).  Whole wave; LDS is in order per wave, so no barrier.
__device__ __forceinline__ void rng_window_hold(RngWindow& rng, uint64_t words, uint32_t lane) {
    if ((rng.pos >> 3) - rng.base_blk >= 64 || rng.pos + words > (rng.base_blk + 64) * 8) {
        rng.base_blk = uni64(rng.pos >> 3);
        uint32_t o[16];
        chacha12_block(rng.seed, rng.base_blk + lane, rng.stream, o);
#pragma unroll
        for (int w = 0; w < 16; ++w) rng.buf[w][lane] = o[w];
    }
}

// Lane j < m draws iteration j of the next m <= 64.  An iteration starts where the earlier ones stopped drawing: a goal sample
// takes its Bernoulli word (plus the disc sampler's two), a uniform sample 1 + dim words.  So the word offset of lane j is
// (1 + dim) j - (dim - gw) popcount(goal lanes below j): the lanes iterate "read my Bernoulli word at the offset implied by
// the current goal mask -> ballot the new goal mask" to its fixed point (after round r the first r lanes are right; one extra
// round per goal sample in the block).  Then `dim` range draws (52-bit transform, res = v01 * scale + lo) follow.
// Lane j hands its sample and the stream position after its draws to store(j, q, pos_after), from registers, and rng.pos then
// moves past the block (store first, as each kernel's own copy did: the other order costs the lanes kernels registers).  A
// rejected range draw (res >= hi) or a block that does not lie inside the window returns false with nothing touched: the caller
// samples that block sequentially.  DISC compiles the disc goal sampler in (D == 2 only, chosen by p.goal_sampler); dim <= D.
template <int D, bool DISC, class Store>
__device__ __forceinline__ bool sample_lanes64(RngWindow& rng, const DevParams& p, int dim, const double* goal_c, double goal_radius,
                                               uint32_t m, uint32_t lane, Store&& store) {
    double q[D];
    const uint32_t per = 1u + (uint32_t)dim;
    const uint64_t win_lo = rng.base_blk * 8;
    const uint64_t pos0 = rng.pos;
    if (pos0 < win_lo || pos0 + (uint64_t)m * per > win_lo + 512) return false;
    const uint32_t rel0 = (uint32_t)(pos0 - win_lo);   // first word of the block inside the window
    const bool act = lane < m;
    const bool always_goal = p.p_int == ~0ull;         // Bernoulli ALWAYS_TRUE: no draw at all
    const bool disc = DISC && D == 2 && p.goal_sampler == OXHIP_GOAL_SAMPLE_UNIFORM_DISC;
    const uint32_t gw = disc ? 2u : 0u;                // words a goal sample draws after its Bernoulli word
    auto word = [&](uint32_t rel) -> uint64_t {        // rel < 512 by the check above
        const uint32_t a = rel0 + rel, bl = a >> 3, w = (a & 7u) * 2u;
        return ((uint64_t)rng.buf[w + 1][bl] << 32) | rng.buf[w][bl];
    };
    uint64_t goal_mask = always_goal ? ~0ull : 0ull;
    uint32_t off = act ? gw * lane : 0u;               // (every iteration is a goal sample: gw words each)
    if (!always_goal) {
        const uint64_t below = below_mask(lane);
        for (uint32_t round = 0; round <= m; ++round) {
            off = act ? per * lane - ((uint32_t)dim - gw) * (uint32_t)__popcll(goal_mask & below) : 0u;
            const uint64_t now = __ballot(act && word(off) < p.p_int);
            if (now == goal_mask) break;
            goal_mask = now;
        }
    }
    const bool goal = (goal_mask >> lane) & 1ull;
    bool redraw = false;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        if (k < dim) {
            const uint64_t bits = (word(act && !goal ? off + 1u + (uint32_t)k : 0u) >> 12) | 0x3FF0000000000000ull;
            const double v01 = __longlong_as_double((long long)bits) - 1.0;
            double res = v01 * p.scale[k];
            res = res + p.lo[k];
            redraw = redraw || !(res < p.hi[k]);
            q[k] = goal ? goal_c[k] : res;
        }
    }
    redraw = redraw && !goal;
    if (DISC && D == 2 && disc) {   // the disc sampler's two words follow the Bernoulli word (if one was drawn)
        const uint32_t base = act && goal ? off + (always_goal ? 0u : 1u) : 0u;
        double gx, gy;
        const bool okd = goal_disc_sample(word(base), word(base + 1u), goal_c, goal_radius, gx, gy);
        if (goal) { q[0] = gx; q[D >= 2 ? 1 : 0] = gy; redraw = !okd; }
    }
    if (__ballot(act && redraw) != 0) return false;
    const uint32_t cnt = always_goal ? gw : (goal ? 1u + gw : per);
    if (act) store(lane, q, pos0 + off + cnt);
    rng.pos = pos0 + (uint32_t)__builtin_amdgcn_readlane((int)(off + cnt), (int)(m - 1));
    return true;
}

// Draws the next m <= 64 iterations: the window hold (`slack` words beyond the block's m (1 + dim)), the lane-parallel attempt,
// and -- after a rejected draw, or for a block the window cannot hold -- the iterations one by one through sample_state.
// store(b, q, pos_after) receives iteration b's sample and the stream position after it: from lane b on the parallel path, from
// lane 0 for b = 0 .. m - 1 in turn on the sequential one (there q and pos_after are wave-uniform).
template <int D, bool DISC, class Store>
__device__ __forceinline__ void sample_block64(RngWindow& rng, const DevParams& p, int dim, const double* goal_c, double goal_radius,
                                               uint32_t m, uint32_t lane, uint32_t slack, Store&& store) {
    rng_window_hold(rng, (uint64_t)m * (1u + (uint32_t)dim) + slack, lane);
    if (!sample_lanes64<D, DISC>(rng, p, dim, goal_c, goal_radius, m, lane, store)) {
        for (uint32_t b = 0; b < m; ++b) {
            double q[D];
            sample_state<D, false>(rng, p, dim, goal_c, q, goal_radius);
            if (lane == 0) store(b, q, rng.pos);
        }
    }
}

}  // namespace oxhip
