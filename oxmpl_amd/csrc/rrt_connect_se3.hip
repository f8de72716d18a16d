// rrt_connect_se3.hip -- RRTConnect (oxmpl/src/geometric/planners/rrt_connect.rs:121-159,166-189,227-309) over
// SE(3) = R^3 x SO(3): a rigid body of spheres among sphere obstacles.
//
// The reference has no SE(3) space (docs/BACKLOG.md:12-14); it is assembled from the reference's components, as SE(2) was
// (rrt_connect_se2.hip), with OMPL's SE(3) weights:
//   (x, y, z)  RealVectorStateSpace  distance rvss.rs:137-155, interpolate :161-186, sample :233-249   (rrt_device.hpp)
//   q          SO3StateSpace         distance, interpolate, sample_uniform                              (so3_device.hpp, so3_sampler.hpp)
//   distance = 1.0 * d_xyz + 1.0 * d_q (one add);  extent = extent_xyz + 0.5 * PI;  interpolate: both parts with the same t
// Validity: body sphere b (centre c_b in the body frame, radius r_b) sits at p = rot(q, c_b) + (x, y, z) in the world; the state
// is valid iff sqrt(|p - o_j|^2) > r_b + r_j for every body sphere and every obstacle (o_j, r_j), strictly.
//   rot(q, v), u = (qx, qy, qz), w = qw:   t = 2 * (u x v);   rot = (v + w * t) + (u x t)
//   with every cross product component evaluated as a*b - c*d (two products, one subtraction) and the two adds left to right.
// All of it in unfused binary64 (-ffp-contract=off), in the order the CPU checker writes it (tests/golden/make_golden_se3.py).
//
// ONE WAVE PER PROBLEM (a 64-thread workgroup, four per CU -- the shape of rrt_connect_se2.hip / rrt_so3.hip).  The first kSe3N
// nodes of BOTH trees are mirrored in LDS (the SoA [7][cap] arrays in HBM receive every store), obstacles and body are staged in
// LDS.  Per extend:
//   nearest   each lane evaluates the exact distance (sqrt + acos) of its strided nodes, strict '<' in ascending index order,
//             then the wave's lexicographic (distance, index) minimum; node 0 survives a NaN as in the reference's scan
//   steer     interpolate(q_near, q, max_distance / min_dist) when min_dist > max_distance
//   motion    the hot part: the interpolated states are computed once each, a lane per state (one SLERP per state), and left in
//             LDS; then the (state, body sphere) pairs are dealt to the lanes -- with few pairs, several lanes share a pair and
//             split the obstacles -- and every lane sweeps its obstacles, without a branch in the sweep (the pairs it cannot
//             clear are decided afterwards).  The verdict is an AND over all (state, body sphere, obstacle) triples, so the
//             dealing cannot change it.
#include "oxhip_internal.hpp"
#include "rrt_device.hpp"
#include "so3_device.hpp"
#include "so3_sampler.hpp"

namespace oxhip {

constexpr int kSe3N = 256;         // nodes of each tree mirrored in LDS (56 B each); beyond that nodes are read from HBM / L2
constexpr int kSe3LdsObs = 128;    // obstacles staged in LDS; larger fields are read from HBM / L2

template <int NO>
struct Se3Scratch {                // what a motion check needs
    double obs[4][NO];             // obstacle centres and radii, SoA (cx, cy, cz, r)
    double body[4][kSe3MaxBody];   // body spheres, SoA (cx, cy, cz, r)
    double st[7][64];              // the interpolated states of the current pass
};
template <int NO>
struct Se3Shared {
    uint32_t rng_buf[16][64];      // the sampler's window: 64 ChaCha12 blocks = 512 words
    double node[2][7][kSe3N];      // the first kSe3N nodes of the start tree and of the goal tree, SoA
    Se3Scratch<NO> mc;
};
static_assert(sizeof(Se3Shared<kSe3LdsObs>) <= 40960, "four problems per CU");

__device__ __forceinline__ void se3_rot(const double q[4], const double v[3], double out[3]) {
    const double a0 = q[1] * v[2], b0 = q[2] * v[1];
    const double a1 = q[2] * v[0], b1 = q[0] * v[2];
    const double a2 = q[0] * v[1], b2 = q[1] * v[0];
    const double tx = 2.0 * (a0 - b0), ty = 2.0 * (a1 - b1), tz = 2.0 * (a2 - b2);
    const double c0 = q[1] * tz, d0 = q[2] * ty;
    const double c1 = q[2] * tx, d1 = q[0] * tz;
    const double c2 = q[0] * ty, d2 = q[1] * tx;
    const double wx = q[3] * tx, wy = q[3] * ty, wz = q[3] * tz;
    double r0 = v[0] + wx, r1 = v[1] + wy, r2 = v[2] + wz;
    out[0] = r0 + (c0 - d0);
    out[1] = r1 + (c1 - d1);
    out[2] = r2 + (c2 - d2);
}
__device__ __forceinline__ double se3_distance(const double a[7], const double b[7]) {
    const double dr = sqrt(dist2<3>(a, b, 3));
    const double dq = so3_distance(a + 3, b + 3);
    return dr + dq;
}
__device__ __forceinline__ void se3_interpolate(const double from[7], const double to[7], double t, double out[7]) {
    lerp<3>(from, to, t, out, 3);
    so3_interpolate(from + 3, to + 3, t, out + 3);
}

// does obstacle (o, ro) touch the body sphere of radius rb at p?  valid iff sqrt(d2) > rb + ro.  The square root is correctly
// rounded and monotone, so d2 > s^2 (1 + 2^-40) with s >= 0 already says "sqrt(d2) > s" (the true root then exceeds s by more than
// 2^-42 s, a quarter of a million ulps): only a pair that close to touching -- or touching -- takes the square root.
__device__ __forceinline__ bool se3_pair_hit(const double p[3], double rb, const double o[3], double ro) {
    const double d2 = dist2<3>(p, o, 3);
    const double s = rb + ro;
    const double s2 = s * s;
    if (s >= 0.0 && d2 > s2 * (1.0 + 0x1p-40)) return false;
    return !(sqrt(d2) > s);
}

template <bool LDS_OBS, class SC>
__device__ __forceinline__ void se3_obstacle(const DevParams& p, const SC& mc, uint32_t j, double o[3], double& ro) {
    if (LDS_OBS) {
        o[0] = mc.obs[0][j]; o[1] = mc.obs[1][j]; o[2] = mc.obs[2][j]; ro = mc.obs[3][j];
    } else {
        const size_t n = p.n_spheres;
        o[0] = p.sph_c[j]; o[1] = p.sph_c[n + j]; o[2] = p.sph_c[2 * n + j]; ro = p.sph_r[j];
    }
}

// is_valid by one lane: every body sphere against every obstacle
template <bool LDS_OBS, class SC>
__device__ __forceinline__ bool se3_state_hit(const DevParams& p, const SC& mc, uint32_t nbody, const double s[7]) {
    bool hit = false;
    for (uint32_t b = 0; b < nbody; ++b) {
        const double c[3] = {mc.body[0][b], mc.body[1][b], mc.body[2][b]};
        const double rb = mc.body[3][b];
        double w[3];
        se3_rot(s + 3, c, w);
        const double pw[3] = {w[0] + s[0], w[1] + s[1], w[2] + s[2]};
        for (uint32_t j = 0; j < p.n_spheres; ++j) {
            double o[3], ro;
            se3_obstacle<LDS_OBS>(p, mc, j, o, ro);
            hit = hit || se3_pair_hit(pw, rb, o, ro);
        }
    }
    return hit;
}

// rrt_connect.rs:166-189 for ONE WAVE; returns the wave-uniform verdict "some tested state is invalid".  The states tested are `to`
// alone (nsteps <= 1) or steps 1 ..= nsteps.  Passes of up to 64 states: lane s interpolates state s into mc.st; then the
// pass's (state, body sphere) pairs are dealt 64 / g at a time, g lanes per pair (g = the largest power of two with pairs * g <= 64,
// 1 when the pairs alone fill the wave), lane k of a pair taking the obstacles k, k + g, ...
template <bool LDS_OBS, class SC>
__device__ __forceinline__ bool se3_motion_invalid_wave(const DevParams& p, SC& mc, uint32_t nbody, const double from[7], const double to[7],
                                                        uint32_t nsteps, uint32_t lane) {
    const uint32_t no = p.n_spheres;
    if (no == 0) return false;
    const uint32_t S = nsteps <= 1u ? 1u : nsteps;
    const double dn = (double)nsteps;
    for (uint32_t s0 = 0; s0 < S;) {
        const uint32_t ch = S - s0 < 64u ? S - s0 : 64u;
        if (lane < ch) {
            double s[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) s[k] = to[k];
            if (nsteps > 1u) se3_interpolate(from, to, (double)(s0 + lane + 1u) / dn, s);
#pragma unroll
            for (int k = 0; k < 7; ++k) mc.st[k][lane] = s[k];
        }
        // the readers below are this wave's own lanes and LDS is in order per wave (the fences keep the compiler from moving the accesses)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const uint32_t npairs = ch * nbody;   // <= 64 * 16
        uint32_t lg = 0;
        while (lg < 6u && (npairs << (lg + 1u)) <= 64u) ++lg;
        const uint32_t g = 1u << lg, per = 64u >> lg;
        const uint32_t sub = lane & (g - 1u);
        bool bad = false;
        for (uint32_t w0 = 0; w0 < npairs; w0 += per) {
            const uint32_t w = w0 + (lane >> lg);
            if (w < npairs) {
                const uint32_t si = w / nbody, b = w - si * nbody;
                const double q[4] = {mc.st[3][si], mc.st[4][si], mc.st[5][si], mc.st[6][si]};
                const double c[3] = {mc.body[0][b], mc.body[1][b], mc.body[2][b]};
                const double rb = mc.body[3][b];
                double r[3];
                se3_rot(q, c, r);
                const double pw[3] = {r[0] + mc.st[0][si], r[1] + mc.st[1][si], r[2] + mc.st[2][si]};
                if (p.dbg_flags & OXHIP_DEBUG_SE3_BRANCHY_SWEEP) {   // the first working kernel's sweep: the decision pair by pair
                    for (uint32_t j = sub; j < no; j += g) {
                        double o[3], ro;
                        se3_obstacle<LDS_OBS>(p, mc, j, o, ro);
                        bad = bad || se3_pair_hit(pw, rb, o, ro);
                    }
                } else {
                    // the sweep without a branch in it (se3_pair_hit's screen alone: the loads and the arithmetic of consecutive
                    // obstacles overlap), remembering the first and last obstacle it could not clear; those few -- a pair that
                    // touches or is within 2^-40 of touching -- are then decided as se3_pair_hit decides them
                    uint32_t jc = 0xFFFFFFFFu, jl = 0u;
#pragma unroll 4
                    for (uint32_t j = sub; j < no; j += g) {
                        double o[3], ro;
                        se3_obstacle<LDS_OBS>(p, mc, j, o, ro);
                        const double d2 = dist2<3>(pw, o, 3);
                        const double s = rb + ro;
                        const double s2 = s * s;
                        const bool clear = s >= 0.0 && d2 > s2 * (1.0 + 0x1p-40);
                        jc = (!clear && jc == 0xFFFFFFFFu) ? j : jc;
                        jl = clear ? jl : j;
                    }
                    if (jc != 0xFFFFFFFFu) {
                        for (uint32_t j = jc; j <= jl; j += g) {
                            double o[3], ro;
                            se3_obstacle<LDS_OBS>(p, mc, j, o, ro);
                            bad = bad || se3_pair_hit(pw, rb, o, ro);
                        }
                    }
                }
            }
        }
        if (__ballot(bad) != 0) return true;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // (the next pass overwrites mc.st)
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        s0 += ch;
    }
    return false;
}

// body (and, when they fit, obstacles) into LDS; the caller synchronises before the first motion check
template <bool LDS_OBS, class SC>
__device__ __forceinline__ void se3_stage(const DevParams& p, const Se3Args& a, SC& mc, uint32_t lane, uint32_t nthreads) {
    for (uint32_t i = lane; i < 4u * (uint32_t)kSe3MaxBody; i += nthreads) (&mc.body[0][0])[i] = a.body[i];
    if (LDS_OBS) {
        const uint32_t no = p.n_spheres;
        for (uint32_t j = lane; j < no; j += nthreads) {
            mc.obs[0][j] = p.sph_c[j]; mc.obs[1][j] = p.sph_c[(size_t)no + j]; mc.obs[2][j] = p.sph_c[2 * (size_t)no + j];
            mc.obs[3][j] = p.sph_r[j];
        }
    }
}

// one tree: SoA [7][cap] in HBM, its first kSe3N nodes in LDS
template <class SH>
__device__ __forceinline__ void se3_load_node(const SH& sh, uint32_t w, const double* tree, size_t cap, uint32_t i, double c[7]) {
    // (two separate sets of loads, the values selected: a pointer that is LDS on one path and HBM on the other would be a flat load)
    const uint32_t il = i < (uint32_t)kSe3N ? i : 0u;
#pragma unroll
    for (int k = 0; k < 7; ++k) c[k] = sh.node[w][k][il];
    if (i >= (uint32_t)kSe3N) {
        double g[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) g[k] = tree[(size_t)k * cap + i];
#pragma unroll
        for (int k = 0; k < 7; ++k) c[k] = g[k];
    }
}

// cycle stamps of problem 0 (diagnostic instantiation, oxhip_rrt_batch_enable_stamps): DevParams::dbg[0..6] = cycles spent sampling, in
// the nearest-neighbour searches, in the steers (with the step count's distance), in the motion checks, in the whole loop;
// iterations; extends
template <bool STAMP>
__device__ __forceinline__ uint64_t se3_clock() { return STAMP ? (uint64_t)__builtin_readcyclecounter() : 0ull; }

// extend() of rrt_connect.rs:121-159 by the whole wave, up to the verdict (no insert); 0 = motion invalid, 1 = Advanced, 2 = Reached
template <bool LDS_OBS, bool STAMP, class SH>
__device__ __forceinline__ int se3_extend_try(const DevParams& p, SH& sh, uint32_t nbody, uint32_t w, const double* tree, size_t cap, uint32_t n,
                                              const double q[7], uint32_t lane, uint32_t& nearest, double q_new[7], uint64_t* acc) {
    const uint64_t t0 = se3_clock<STAMP>();
    // nearest (rrt_connect.rs:128-136): lexicographic (distance, index) minimum; a NaN distance of node 0 keeps node 0 (every later
    // comparison with it fails), a NaN elsewhere never wins
    const uint32_t n_lds = n < (uint32_t)kSe3N ? n : (uint32_t)kSe3N;
    Exact e{__builtin_inf(), 0xFFFFFFFFu};
    double d0 = 0.0;
    for (uint32_t i = lane; i < n_lds; i += 64u) {
        double c[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) c[k] = sh.node[w][k][i];
        const double d = se3_distance(c, q);
        if (i == 0) d0 = d;
        if (d < e.dist) { e.dist = d; e.idx = i; }
    }
    for (uint32_t i = n_lds + lane; i < n; i += 64u) {   // nodes beyond the mirror (indices keep ascending within a lane)
        double c[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) c[k] = tree[(size_t)k * cap + i];
        const double d = se3_distance(c, q);
        if (d < e.dist) { e.dist = d; e.idx = i; }
    }
    e = exact_wave_reduce(e);
    d0 = readlane_f64(d0, 0);
    nearest = e.idx;
    double min_dist = e.dist;
    if (d0 != d0 || nearest == 0xFFFFFFFFu) { nearest = 0; min_dist = d0; }
    nearest = uni(nearest);
    double q_near[7];
    se3_load_node(sh, w, tree, cap, nearest, q_near);
    const uint64_t t1 = se3_clock<STAMP>();
    // steer (rrt_connect.rs:140-147) and the step count of check_motion
    int result;
    uint32_t nsteps;
    if (min_dist > p.max_distance) {
        se3_interpolate(q_near, q, p.max_distance / min_dist, q_new);
        nsteps = num_steps_u32(se3_distance(q_near, q_new), p.res);
        result = 1;
    } else {
#pragma unroll
        for (int k = 0; k < 7; ++k) q_new[k] = q[k];
        nsteps = num_steps_u32(min_dist, p.res);   // distance(q_near, q): the value the scan computed for this very pair
        result = 2;
    }
    const uint64_t t2 = se3_clock<STAMP>();
    const bool invalid = se3_motion_invalid_wave<LDS_OBS>(p, sh.mc, nbody, q_near, q_new, nsteps, lane);
    if (STAMP) { acc[1] += t1 - t0; acc[2] += t2 - t1; acc[3] += se3_clock<STAMP>() - t2; acc[6] += 1; }
    return invalid ? 0 : result;
}

// tree.push of rrt_connect.rs:150-157
template <class SH>
__device__ __forceinline__ void se3_insert(SH& sh, uint32_t w, double* tree, int32_t* parent, size_t cap, uint32_t& n, uint32_t nearest,
                                           const double q_new[7], uint32_t lane) {
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 7; ++k) tree[(size_t)k * cap + n] = q_new[k];
        parent[n] = (int32_t)nearest;
        if (n < (uint32_t)kSe3N) {
#pragma unroll
            for (int k = 0; k < 7; ++k) sh.node[w][k][n] = q_new[k];
        }
    }
    // the next scan is this wave's own and LDS is in order per wave (the fences keep the compiler from moving the store)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    ++n;
}

template <bool LDS_OBS, bool STAMP>
__global__ __launch_bounds__(64) void rrt_connect_se3_kernel(DevParams p, Se3Args a) {
    const uint32_t prob = blockIdx.x, lane = threadIdx.x;
    __shared__ Se3Shared<LDS_OBS ? kSe3LdsObs : 1> sh;
    ProblemState st = p.state[prob];
    if (st.goal_node >= 0) return;   // already solved: solve() is idempotent
    const uint32_t nbody = a.n_body;
    se3_stage<LDS_OBS>(p, a, sh.mc, lane, 64u);
    const size_t cap = p.cap;
    double* tree_a = p.tree + (size_t)prob * 7 * cap;
    double* tree_b = p.tree_b + (size_t)prob * 7 * cap;
    int32_t* par_a = p.parent + (size_t)prob * cap;
    int32_t* par_b = p.parent_b + (size_t)prob * cap;
    double goal_c[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) goal_c[k] = p.goal_c[(size_t)prob * 7 + k];
    const double goal_radius = p.goal_thr[prob];   // the radius itself: the goal test compares the SE(3) distance

    uint32_t na = st.n_nodes, nb = st.n_nodes_b;
    for (uint32_t i = lane; i < na && i < (uint32_t)kSe3N; i += 64u) {   // a solve call continues the trees an earlier one left in HBM
#pragma unroll
        for (int k = 0; k < 7; ++k) sh.node[0][k][i] = tree_a[(size_t)k * cap + i];
    }
    for (uint32_t i = lane; i < nb && i < (uint32_t)kSe3N; i += 64u) {
#pragma unroll
        for (int k = 0; k < 7; ++k) sh.node[1][k][i] = tree_b[(size_t)k * cap + i];
    }
    RngWindow rng;
    rng.init(sh.rng_buf, p.seed, p.first_problem_id + prob, st.draws);
    __syncthreads();

    int32_t stop = 1;   // OXHIP_STOP_ITERATIONS
    uint64_t h = uni64(st.checksum);
    uint64_t acc[7] = {0, 0, 0, 0, 0, 0, 0};
    const uint64_t t_begin = se3_clock<STAMP>();
    for (uint64_t it = 0; it < p.budget; ++it) {
        if (na >= p.max_nodes || nb >= p.max_nodes) { stop = 2; break; }   // the node cap is looked at before any draw
        const bool gs = na <= nb;   // rrt_connect.rs:249-254: grow the smaller tree
        const uint64_t ts = se3_clock<STAMP>();

        // sample (rrt_connect.rs:258-262): random_bool; the goal's centre, or x, y, z by random_range and then SO(3)'s sampler
        double q[7];
        bool goal;
        if (p.p_int == ~0ull) goal = true;              // Bernoulli ALWAYS_TRUE: no draw
        else goal = rng.next<false>() < p.p_int;        // one u64
        if (goal) {
#pragma unroll
            for (int k = 0; k < 7; ++k) q[k] = goal_c[k];
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                double res;
                for (;;) {
                    const uint64_t bits = (rng.next<false>() >> 12) | 0x3FF0000000000000ull;
                    const double v01 = __longlong_as_double((long long)bits) - 1.0;
                    res = v01 * p.scale[k];
                    res = res + p.lo[k];
                    if (res < p.hi[k]) break;   // else draw again (rand's sample_single loop)
                }
                q[k] = res;
            }
            so3_sample_uniform_wave(rng, p, lane, q + 3);
        }
        if (STAMP) { acc[0] += se3_clock<STAMP>() - ts; acc[5] += 1; }

        // first extend: the tree that grows towards the sample
        uint32_t near_a = 0;
        double qa[7];
        const int ra = se3_extend_try<LDS_OBS, STAMP>(p, sh, nbody, gs ? 0u : 1u, gs ? tree_a : tree_b, cap, gs ? na : nb, q, lane, near_a, qa, acc);
        h = fnv_mix(h, gs ? 1ull : 0ull);
        h = fnv_mix(h, (uint64_t)near_a);
#pragma unroll
        for (int k = 0; k < 7; ++k) h = fnv_mix(h, (uint64_t)__double_as_longlong(qa[k]));
        h = fnv_mix(h, (uint64_t)ra);
        st.iterations++;
        if (ra == 0) continue;
        if (gs) se3_insert(sh, 0u, tree_a, par_a, cap, na, near_a, qa, lane);
        else se3_insert(sh, 1u, tree_b, par_b, cap, nb, near_a, qa, lane);
        const uint32_t idx_a = (gs ? na : nb) - 1u;
        if (gs && se3_distance(qa, goal_c) <= goal_radius) {   // rrt_connect.rs:271-274
            st.goal_node = (int32_t)idx_a;
            st.goal_node_b = -1;
            stop = 0;
            break;
        }
        // ONE extend of the other tree towards the new node; splice on Reached (rrt_connect.rs:277-305)
        uint32_t near_b = 0;
        double qb[7];
        const int rb = se3_extend_try<LDS_OBS, STAMP>(p, sh, nbody, gs ? 1u : 0u, gs ? tree_b : tree_a, cap, gs ? nb : na, qa, lane, near_b, qb, acc);
        h = fnv_mix(h, (uint64_t)near_b);
#pragma unroll
        for (int k = 0; k < 7; ++k) h = fnv_mix(h, (uint64_t)__double_as_longlong(qb[k]));
        h = fnv_mix(h, (uint64_t)rb);
        if (rb != 0) {
            if (gs) se3_insert(sh, 1u, tree_b, par_b, cap, nb, near_b, qb, lane);
            else se3_insert(sh, 0u, tree_a, par_a, cap, na, near_b, qb, lane);
        }
        if (rb == 2) {
            const uint32_t idx_b = (gs ? nb : na) - 1u;
            st.goal_node = (int32_t)(gs ? idx_a : idx_b);
            st.goal_node_b = (int32_t)(gs ? idx_b : idx_a);
            stop = 0;
            break;
        }
    }
    if (STAMP && prob == 0 && lane == 0 && p.dbg) {
        acc[4] = se3_clock<STAMP>() - t_begin;
        for (int k = 0; k < 7; ++k) p.dbg[k] = acc[k];
    }
    if (lane == 0) {
        st.checksum = h;
        st.n_nodes = na;
        st.n_nodes_b = nb;
        st.draws = rng.pos;
        st.stop_reason = stop;
        p.state[prob] = st;
    }
}

uint32_t se3_lds_obstacles() { return (uint32_t)kSe3LdsObs; }

void launch_rrt_connect_se3(const DevParams& p, const Se3Args& a, hipStream_t stream) {
    const dim3 grid(p.n_problems), block(64);
    const bool lds = p.n_spheres <= (uint32_t)kSe3LdsObs;
    if (p.dbg) {   // diagnostic instantiation (cycle stamps of problem 0)
        if (lds) hipLaunchKernelGGL((rrt_connect_se3_kernel<true, true>), grid, block, 0, stream, p, a);
        else hipLaunchKernelGGL((rrt_connect_se3_kernel<false, true>), grid, block, 0, stream, p, a);
        return;
    }
    if (lds) hipLaunchKernelGGL((rrt_connect_se3_kernel<true, false>), grid, block, 0, stream, p, a);
    else hipLaunchKernelGGL((rrt_connect_se3_kernel<false, false>), grid, block, 0, stream, p, a);
}

// ---- stand-alone primitives (parity tests of the SE(3) arithmetic and of the checker)
__global__ void se3_op_kernel(uint32_t op, const double* a, const double* b, const double* t, uint32_t n, double* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double x[7], y[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) { x[k] = a[7 * (size_t)i + k]; y[k] = b[7 * (size_t)i + k]; }
    if (op == 0) { out[i] = se3_distance(x, y); return; }
    if (op == 1) {
        double o[7];
        se3_interpolate(x, y, t[i], o);
#pragma unroll
        for (int k = 0; k < 7; ++k) out[7 * (size_t)i + k] = o[k];
        return;
    }
    double r[3];
    se3_rot(x + 3, y, r);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[3 * (size_t)i + k] = r[k] + x[k];
}
void launch_se3_op(uint32_t op, const double* a, const double* b, const double* t, uint32_t n, double* out, hipStream_t s) {
    hipLaunchKernelGGL(se3_op_kernel, dim3((n + 255) / 256), dim3(256), 0, s, op, a, b, t, n, out);
}

__global__ __launch_bounds__(256) void se3_is_valid_kernel(DevParams p, Se3Args a, const double* states, uint32_t n, uint8_t* out) {
    __shared__ Se3Scratch<1> mc;
    se3_stage<false>(p, a, mc, threadIdx.x, 256u);
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) s[k] = states[7 * (size_t)i + k];
    out[i] = se3_state_hit<false>(p, mc, a.n_body, s) ? 0 : 1;
}
void launch_se3_is_valid(const DevParams& p, const Se3Args& a, const double* states, uint32_t n, uint8_t* out, hipStream_t s) {
    hipLaunchKernelGGL(se3_is_valid_kernel, dim3((n + 255) / 256), dim3(256), 0, s, p, a, states, n, out);
}

// one wave per motion
__global__ __launch_bounds__(64) void se3_check_motion_kernel(DevParams p, Se3Args a, const double* from, const double* to, uint32_t n,
                                                               uint8_t* out) {
    __shared__ Se3Scratch<1> mc;
    const uint32_t m = blockIdx.x, lane = threadIdx.x;
    se3_stage<false>(p, a, mc, lane, 64u);
    __syncthreads();
    if (m >= n) return;
    double f[7], g[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) { f[k] = from[7 * (size_t)m + k]; g[k] = to[7 * (size_t)m + k]; }
    const bool any = se3_motion_invalid_wave<false>(p, mc, a.n_body, f, g, num_steps_u32(se3_distance(f, g), p.res), lane);
    if (lane == 0) out[m] = any ? 0 : 1;
}
void launch_se3_check_motion(const DevParams& p, const Se3Args& a, const double* from, const double* to, uint32_t n, uint8_t* out, hipStream_t s) {
    hipLaunchKernelGGL(se3_check_motion_kernel, dim3(n), dim3(64), 0, s, p, a, from, to, n, out);
}

}  // namespace oxhip
