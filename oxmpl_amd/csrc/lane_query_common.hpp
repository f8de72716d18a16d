// lane_query_common.hpp -- what the lane-per-query kernels (rrt_lanes.hip, rrt_cells.hip) share.  First the small helpers:
// bit casts, in-place minima, wave-wide 64-bit sums, the two-instruction screen verdict, lane masks, the screens' error bound.
// Then the steps of a round that carry the reference's semantics, each stated once: a new node as the binary32 screens hold
// it, every lane's own motion check, the round's checksum, and the whole-tree path of one ambiguous query -- its memo, the d2
// scan, the literal loop and the motion check by the whole wave (rrt_resident.hip takes the last two as well).
// rrt_cells.hip calls every one of them (the motion check in its table form, motion_own_lane_short, which falls back to
// motion_own_lane).  rrt_lanes.hip calls the lanes' own motion check -- motion_own_lane: its callback runs once per step of the
// longest motion, which the table form's loop order does not offer -- and keeps its own text of the other
// steps, each on a measured figure (profiles/lane_query_shared/README.md): growing trees ran slower with the d2 scan shared
// (R^5 -5.3 %: the register allocation around the hot loop moves with the text of the rare path), with the literal loop or the
// wave-wide motion check (R^5 -1.1 % each), with the checksum (R^5 -1.4 %), and with the binary32 node, the memo and
// readlane_u64 together (R^4 -1.6 %).
#pragma once

#include "rrt_device.hpp"
#include "rrt_resident_common.hpp"

namespace oxhip {

typedef float lf32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t lf32_bits(float v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ float lbits_f32(uint32_t v) { return __builtin_bit_cast(float, v); }

__device__ __forceinline__ void vmin_f32(float& acc, float x) {   // plain v_min_f32 in place: no canonicalising v_max in front,
    asm("v_min_f32 %0, %0, %1" : "+v"(acc) : "v"(x));             // and no renamed register to copy back where branches join
}
__device__ __forceinline__ void vmin3_f32(float& acc, float x, float y) {   // acc = min(acc, x, y) in one issue slot (never NaN here)
    asm("v_min3_f32 %0, %0, %1, %2" : "+v"(acc) : "v"(x), "v"(y));
}

// wave-wide sum of a 64-bit value (mod 2^64); every lane of the last row holds it, lane 63 is read
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint64_t dpp_add_step(uint64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, ROW_MASK, 0xf, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, ROW_MASK, 0xf, false);
    return v + (((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
    v = dpp_add_step<0xB1, 0xf>(v);    // quad_perm [1,0,3,2]
    v = dpp_add_step<0x4E, 0xf>(v);    // quad_perm [2,3,0,1]
    v = dpp_add_step<0x141, 0xf>(v);   // row_half_mirror
    v = dpp_add_step<0x140, 0xf>(v);   // row_mirror: every lane holds its row's sum
    v = dpp_add_step<0x142, 0xa>(v);   // row_bcast:15 into rows 1, 3
    v = dpp_add_step<0x143, 0xc>(v);   // row_bcast:31 into rows 2, 3: lane 63 holds the total
    return readlane_u64(v, 63);
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) { return ~wave_min_u32(~v); }
__device__ __forceinline__ double wave_max_f64pos(double v) {   // v >= +0 (or NaN -> treated as huge): bit patterns order like values
    const uint32_t hi = wave_max_u32((uint32_t)__double2hiint(v));
    const uint32_t lo = wave_max_u32((uint32_t)__double2hiint(v) == hi ? (uint32_t)__double2loint(v) : 0u);
    return __hiloint2double((int)hi, (int)lo);
}
__device__ __forceinline__ float f32_up(double x) {   // a binary32 value >= x (two ulps of slack; NaN stays NaN, +inf stays +inf)
    const float t = (float)x;
    return t + fabsf(t) * 0x1p-22f + 1e-37f;
}

// bits <- 2 bits + [!(sp > thr)]: a screen verdict shifted into a lane's bit string in two instructions (compare into vcc,
// add-with-carry of the string to itself); NaN counts as "look".  After eight calls verdict t sits at bit 7 - t.
__device__ __forceinline__ void screen_bit(uint32_t& bits, float sp, float thr) {
    asm("v_cmp_ngt_f32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(bits) : "v"(sp), "v"(thr) : "vcc");
}
__device__ __forceinline__ uint32_t rev8(uint32_t bits) { return __brev(bits) >> 24; }   // verdict t back at bit t
__device__ __forceinline__ uint64_t first_n_mask(uint32_t n) { return n >= 64u ? ~0ull : ((1ull << n) - 1ull); }


struct LMargins {
    double e2;        // 2E: twice the bound on |s' + |b|^2 - d^2| of the dot-product screen (E = u H^2 D (3D + 9), rrt_lanes.hip)
    bool usable;      // H small enough for binary32 products
};

// E of the dot-product screen (rrt_lanes.hip's error model) for a magnitude bound h relative to c0.  u H^2 D (3D + 9) holds while
// binary32 results are normal; below 2^-126 a rounding errs by up to 2^-150 whatever the value, so each of the D + 1 binary32
// roundings of s' (cc and the D fused multiply-adds) adds 2^-150 and the conversions fl32(x - c0), fl32(q - c0) add 2^-150 per
// coordinate, at most 4 D H 2^-149 in d^2 -- below (D + 1) 2^-150 for H < 1/8, and below the 1.0001 slack of the first term
// above: (D + 1) 2^-149 covers both.  (Without it a scene of extent ~1e-22 gets screen values whose rounding is coarser than
// E, and a screen verdict can name the wrong nearest node.)  1e-290: binary64 underflow of h * h and |b|^2.
__device__ __forceinline__ double lanes_screen_e(double h, int dim) {
    return 0x1p-24 * h * h * (double)(dim * (3 * dim + 9)) * 1.0001 + 1e-290 + (double)(dim + 1) * 0x1p-149;
}

// ---------------------------------------------------------------- a new node as the binary32 screens hold it
// a = fl32(qn - c0) and cc = fl32(|a|^2), the sum in binary64
template <int D>
__device__ __forceinline__ void node_f32(const double (&qn)[D], const double (&c0)[D], float (&a)[D], float& cc) {
    double sq = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        a[k] = (float)(qn[k] - c0[k]);
        sq += (double)a[k] * (double)a[k];
    }
    cc = (float)sq;
}

// ---------------------------------------------------------------- every lane's own motion check (rrt.rs:90-116)
// obs: the first 64 spheres in LDS -- rows 0 .. D-1 the centres, row D the squared radius, row D + 1 the midpoint filter's
// threshold.  The binary64 midpoint filter over the spheres a lane's pre-screen left (per lane: usually none or one): the
// subset of `cand` that the motion around `mid` can touch at all.
template <int D>
__device__ __forceinline__ uint64_t spheres_maybe_hit(const double (&obs)[D + 2][64], uint64_t cand, const double (&mid)[D]) {
    uint64_t rem = cand, keep = 0;
    while (__ballot(rem != 0) != 0) {   // two candidates per trip: both spheres are on their way before either is tested
        const uint64_t rem1 = rem & (rem - 1);
        const bool has0 = rem != 0, has1 = rem1 != 0;
        const uint32_t o0 = has0 ? (uint32_t)(__ffsll((unsigned long long)rem) - 1) : 0u;
        const uint32_t o1 = has1 ? (uint32_t)(__ffsll((unsigned long long)rem1) - 1) : 0u;
        double c0[D], c1[D];
#pragma unroll
        for (int k = 0; k < D; ++k) { c0[k] = obs[k][o0]; c1[k] = obs[k][o1]; }
        const double f0 = obs[D + 1][o0], f1 = obs[D + 1][o1];
        if (has0 && sphere_maybe_hit<D>(c0, f0, mid)) keep |= 1ull << o0;
        if (has1 && sphere_maybe_hit<D>(c1, f1, mid)) keep |= 1ull << o1;
        rem = rem1 & (rem1 - 1);
    }
    return keep;
}
// ... and every lane with `need` steps through its own motion against just the spheres of `maybe` (is_valid is pure: testing
// all states equals the reference's first-invalid early exit), and against every obstacle beyond the first 64.  Returns
// "found an invalid state".  each_step(s) runs once per step of the longest motion (wave-uniform s).
template <int D, class F>
__device__ __forceinline__ bool motion_own_lane(const DevParams& p, const double (&obs)[D + 2][64], bool need, uint64_t maybe, const double (&q_near)[D],
                                                const double (&qn)[D], uint32_t ns64, uint32_t nobs, F&& each_step) {
    bool bad = false;
    if (__ballot(need) != 0) {
        const double dist = sqrt(dist2<D>(q_near, qn, D));
        const uint32_t nsteps = num_steps_u32(dist, p.res);
        const uint32_t steps_l = need ? (nsteps <= 1 ? 1u : nsteps) : 0u;
        const uint32_t smax = wave_max_u32(steps_l);
        const double dn = (double)nsteps;
        for (uint32_t s = 1; s <= smax && s != 0; ++s) {
            const bool on = s <= steps_l;
            double x[D];
            {
                const double t = (double)s / dn;
                double xi[D];
                lerp<D>(q_near, qn, t, xi, D);
#pragma unroll
                for (int k = 0; k < D; ++k) x[k] = nsteps <= 1 ? qn[k] : xi[k];   // num_steps <= 1: is_valid(to) only
            }
            uint64_t rem = on ? maybe : 0ull;
            while (__ballot(rem != 0) != 0) {
                const bool has = rem != 0;
                const uint32_t o = has ? (uint32_t)(__ffsll((unsigned long long)rem) - 1) : 0u;
                double c[D];
#pragma unroll
                for (int k = 0; k < D; ++k) c[k] = obs[k][o];
                bad = bad || (has && !(dist2<D>(c, x, D) > obs[D][o]));
                rem &= rem - 1;
            }
            for (uint32_t jx = ns64; jx < nobs; ++jx) bad = bad || (on && obstacle_hit<D>(p, D, x, jx));
            each_step(s);
        }
    }
    return bad;
}

// The step fractions of short motions, t[n - 1][s - 1] = (double)s / (double)n for 1 <= s <= n <= kStepTabMax, in LDS: the
// quotients of the loop above by the device's own binary64 division, so their bits are the ones that loop computes.  Filled
// by the first 64 threads of the workgroup before its barrier.
constexpr uint32_t kStepTabMax = 8;
struct StepFractions { double t[kStepTabMax][kStepTabMax]; };
__device__ __forceinline__ void step_fractions_fill(StepFractions& tab, uint32_t tid) {
    if (tid < kStepTabMax * kStepTabMax) tab.t[tid >> 3][tid & 7u] = (double)((tid & 7u) + 1u) / (double)((tid >> 3) + 1u);
}
// motion_own_lane with the loops interchanged where the order is free: the spheres of `maybe` outside -- a sphere is read
// from LDS once, as many trips as the fullest lane has bits -- and the steps inside, t from the table (no division; the next
// step's t is on its way while this step is tested).  The obstacles beyond the first 64 keep their loop over the steps.  A
// wave in which a motion has more than kStepTabMax steps takes motion_own_lane as it is.
template <int D>
__device__ __forceinline__ bool motion_own_lane_short(const DevParams& p, const double (&obs)[D + 2][64], const StepFractions& tab, bool need, uint64_t maybe,
                                                      const double (&q_near)[D], const double (&qn)[D], uint32_t ns64, uint32_t nobs) {
    if (__ballot(need) == 0) return false;
    const double dist = sqrt(dist2<D>(q_near, qn, D));
    const uint32_t nsteps = num_steps_u32(dist, p.res);
    const uint32_t steps_l = need ? (nsteps <= 1 ? 1u : nsteps) : 0u;
    const uint32_t smax = wave_max_u32(steps_l);
    if (smax > kStepTabMax) return motion_own_lane<D>(p, obs, need, maybe, q_near, qn, ns64, nobs, [](uint32_t) {});
    const double* trow = tab.t[(steps_l == 0 ? 1u : steps_l) - 1u];   // (a lane without `need` reads row 0 and tests nothing)
    auto state = [&](double t, double (&x)[D]) {
        double xi[D];
        lerp<D>(q_near, qn, t, xi, D);
#pragma unroll
        for (int k = 0; k < D; ++k) x[k] = nsteps <= 1 ? qn[k] : xi[k];   // num_steps <= 1: is_valid(to) only
    };
    bool bad = false;
    uint64_t rem = need ? maybe : 0ull;
    while (__ballot(rem != 0) != 0) {
        const bool has = rem != 0;
        const uint32_t o = has ? (uint32_t)(__ffsll((unsigned long long)rem) - 1) : 0u;
        double c[D];
#pragma unroll
        for (int k = 0; k < D; ++k) c[k] = obs[k][o];
        const double thr = obs[D][o];
        double t_next = trow[0];
        for (uint32_t s = 1; s <= smax; ++s) {
            const double t = t_next;
            t_next = trow[s < kStepTabMax ? s : kStepTabMax - 1u];
            double x[D];
            state(t, x);
            bad |= (bool)((int)has & (int)(s <= steps_l) & (int)!(dist2<D>(c, x, D) > thr));   // (no short circuit: the steps overlap)
        }
        rem &= rem - 1;
    }
    if (ns64 < nobs) {
        for (uint32_t s = 1; s <= smax; ++s) {
            double x[D];
            state(trow[s - 1u], x);
            for (uint32_t jx = ns64; jx < nobs; ++jx) bad = bad || (s <= steps_l && obstacle_hit<D>(p, D, x, jx));
        }
    }
    return bad;
}

// ---------------------------------------------------------------- the round's checksum
// P^lane for the batched checksum (H <- H P^m + sum_j g_j P^(m-1-j)); P^64 for a full batch is chk_lane_power(..)[63] * P
__device__ __forceinline__ uint64_t chk_lane_power(uint32_t lane) {
    uint64_t pw = 1, base = kFnvPrime;
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        if ((lane >> b) & 1u) pw *= base;
        base *= base;
    }
    return pw;
}
// H <- H P^cut + sum_{j < cut} g_j P^(cut-1-j) over the lanes [0, cut) that are `counted` (g_j: the lane's own iteration)
template <int D>
__device__ __forceinline__ uint64_t chk_push_round(uint64_t h, uint64_t pw, uint64_t pw64, uint32_t lane, uint32_t cut, bool counted, uint32_t nearest,
                                                   const double (&qn)[D], bool ok) {
    const bool mine = lane < cut;
    const uint64_t gd = iter_digest<D>(nearest, qn, D, ok);
    const int src = mine ? (int)(cut - 1u - lane) : 0;
    // (src < 64: the permute itself, without __shfl's own lane number -- one more register held across the rounds)
    const uint64_t w = ((uint64_t)(uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)(uint32_t)(pw >> 32)) << 32) |
                       (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)(uint32_t)pw);
    const uint64_t sum = wave_sum_u64((mine && counted) ? gd * w : 0ull);
    const uint64_t pc = cut >= 64u ? pw64 : readlane_u64(pw, (int)cut);
    return h * pc + sum;
}

// ---------------------------------------------------------------- the whole-tree path: one ambiguous query, the whole wave
// The last whole-tree answer, four variables of the kernel: memo_idx is the exact nearest node, at squared distance memo_g, the
// minimum unique, of query memo_q for the tree of memo_n nodes.  A fixed query on an unchanged tree has a fixed answer: the goal
// centre is drawn again and again -- goal_bias -- and when the screen cannot decide it once, it cannot decide it the next time
// either.  (Four variables, not a struct: as a struct the growing R^3 cells kernel came out with a 36-byte private segment.)
template <int D>
__device__ __forceinline__ bool memo_matches(uint32_t memo_n, const double (&memo_q)[D], uint32_t n, const double (&q)[D]) {
    bool same = memo_n == n;
#pragma unroll
    for (int k = 0; k < D; ++k) same = same && __double_as_longlong(q[k]) == __double_as_longlong(memo_q[k]);   // bit for bit
    return same;
}
template <int D>
__device__ __forceinline__ void memo_keep(uint32_t& memo_n, double (&memo_q)[D], double& memo_g, uint32_t& memo_idx, uint32_t n, const double (&q)[D],
                                          double g, uint32_t idx) {
    memo_n = n; memo_g = g; memo_idx = idx;
#pragma unroll
    for (int k = 0; k < D; ++k) memo_q[k] = q[k];
}

// One query against every node by squared distances, the wave striding over the tree: a lane takes four consecutive nodes
// per 32-byte load and coordinate, WT such chunks of 256 nodes per trip -- 4 WT nodes per lane in flight (the trees of a whole
// batch do not fit the L2: a trip is a DRAM / Infinity Cache round trip).  If exactly one node is within a rounding of the
// minimum gmin, it is the reference's nearest node `idx` (sqrt is monotone).  Returns true for a genuine near-tie -- two d2
// that may share a correctly rounded root; idx is then kNoNode and the literal loop below decides.
template <int D, int WT>
__device__ __forceinline__ bool whole_tree_nearest(const double* tree, const uint8_t* skip, size_t cap, uint32_t n, uint32_t lane, const double (&q)[D],
                                                   double& gmin, uint32_t& idx) {
    typedef double ldouble4 __attribute__((ext_vector_type(4)));
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // this wave's stores to the tree have landed (same CU)
    Scan ps{__builtin_inf(), kNoNode, 0xFFFFFFFFu};  // .slot is used as the node index here
    for (uint32_t i0 = 4u * lane; i0 < n; i0 += 256u * (uint32_t)WT) {
        uint32_t sk4[WT], il[WT];
        double d16[WT][4];
#pragma unroll
        for (int t = 0; t < WT; ++t) {
            const uint32_t ib = i0 + 256u * (uint32_t)t;
            il[t] = ib < n ? ib : 0u;   // (rows are padded to cap >= n rounded up to 1024)
            sk4[t] = *reinterpret_cast<const uint32_t*>(skip + il[t]);
        }
#pragma unroll
        for (int k = 0; k < D; ++k) {
            ldouble4 ck[WT];
#pragma unroll
            for (int t = 0; t < WT; ++t) ck[t] = *reinterpret_cast<const ldouble4*>(tree + (size_t)k * cap + il[t]);
#pragma unroll
            for (int t = 0; t < WT; ++t) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double df = ck[t][r] - q[k];
                    const double sq = df * df;
                    d16[t][r] = k == 0 ? sq : d16[t][r] + sq;   // the reference's summation order
                }
            }
        }
#pragma unroll
        for (int t = 0; t < WT; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t i = i0 + 256u * (uint32_t)t + (uint32_t)r;
                if (i < n && ((sk4[t] >> (8 * r)) & 0xFFu) == 0) scan_push(ps, d16[t][r], i);   // ascending within the lane: ties keep the lower index
            }
        }
    }
    gmin = wave_min_f64(ps.b1);
    const uint32_t hbw = hi32(gmin) + 1;
    const uint64_t nearm = __ballot(ps.slot != kNoNode && hi32(ps.b1) <= hbw);
    const bool tie = __popcll(nearm) != 1 || __ballot(ps.h2 <= hbw) != 0;
    idx = tie ? kNoNode : (uint32_t)__builtin_amdgcn_readlane((int)ps.slot, __ffsll((unsigned long long)(nearm | (1ull << 63))) - 1);
    return tie;
}

// The reference's literal loop (rrt.rs:187-196: post-sqrt compare, strict '<', lowest index among ties) over the persistent
// copy of the tree in global memory.  Returns the distance; nearest and q_near are the winner's (all wave-uniform).
template <int D>
__device__ __forceinline__ double literal_nearest(const double* tree, size_t cap, uint32_t n, uint32_t lane, const double (&q)[D], uint32_t& nearest,
                                                  double (&q_near)[D]) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    Exact e{__builtin_inf(), kNoNode};
    for (uint32_t i = lane; i < n; i += 64) {
        double c[D];
#pragma unroll
        for (int k = 0; k < D; ++k) c[k] = __hip_atomic_load(&tree[(size_t)k * cap + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const double d = sqrt(dist2<D>(c, q, D));
        if (d < e.dist) { e.dist = d; e.idx = i; }
    }
    e = exact_wave_reduce(e);
    nearest = uni(e.idx);
#pragma unroll
    for (int k = 0; k < D; ++k) q_near[k] = unid(__hip_atomic_load(&tree[(size_t)k * cap + nearest], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    return unid(e.dist);
}

// check_motion (rrt.rs:90-116) of one query's motion by the whole wave: lane s holds sphere s (oc, othr, ofilt); `extras`:
// there are obstacles beyond the first 64 spheres.  The midpoint filter first: usually no sphere can be touched at all.
template <int D>
__device__ __forceinline__ bool motion_wave(const DevParams& p, uint32_t lane, const double (&q_near)[D], const double (&q_new)[D], const double (&oc)[D],
                                            double othr, double ofilt, uint32_t ns64, bool extras) {
    double mid[D];
    lerp<D>(q_near, q_new, 0.5, mid, D);
    if (__ballot(sphere_maybe_hit<D>(oc, ofilt, mid)) == 0 && !extras) return true;
    return motion_lanes<D>(p, lane, q_near, q_new, oc, othr, ofilt, ns64);
}

}  // namespace oxhip
