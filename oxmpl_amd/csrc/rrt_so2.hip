// rrt_so2.hip -- RRT (oxmpl/src/geometric/planners/rrt.rs:170-225) over SO2StateSpace (one angle per state,
// oxmpl/src/base/spaces/so2_state_space.rs) with the forbidden-arc checker of the reference's SO(2) fixture
// (oxmpl/tests/rrt_so2ss_tests.rs, ForbiddenAngleChecker).  Arithmetic: so2_device.hpp.
//
// ONE WAVE PER PROBLEM (a 64-thread workgroup, four per CU -- the shape of rrt_so3.hip): an iteration is a chain of dependent
// steps, so what counts is the length of that chain.  The tree lives in HBM as SoA [1][cap] (every store lands there) and its
// first kSo2N nodes are mirrored in LDS; the arcs are staged in LDS when they fit.  Per iteration:
//   sample    64 iterations' samples at a time through the lane-parallel sampler (lane_sampler.hpp, dim = 1: the Bernoulli word,
//             then one range draw), kept in LDS with the stream position after each of them: a launch that stops inside a block
//             leaves `draws` where the sequential loop leaves it
//   nearest   each lane computes the exact distance of its strided nodes, strict '<' in ascending index order, then the wave's
//             lexicographic (distance, index) minimum: the reference's argmin with the lowest index among ties.  No binary32 screen.
//   steer     interpolate(q_near, q_rand, max_distance / min_dist) when min_dist > max_distance, else q_new = q_rand bit for bit
//             (rrt.rs:199-208: not normalised)
//   motion    the interpolated states of check_motion (rrt.rs:90-116) are dealt to the lanes, 64 per pass, each against every arc
//   insert    lane 0 stores node n (HBM + LDS mirror), then the goal test distance(q_new, target) <= radius
// The checksum is the per-iteration polynomial of ABI 2 (rrt_device.hpp, iter_digest) over the one coordinate.
// The wave-local fence and the motion pass are rrt_wave.hpp's, shared with rrt_so3.hip.
#include "oxhip_internal.hpp"
#include "rrt_device.hpp"
#include "lane_sampler.hpp"
#include "so2_device.hpp"
#include "rrt_wave.hpp"

namespace oxhip {

constexpr int kSo2N = 4096;       // tree nodes mirrored in LDS (8 B each); beyond that nodes are read from HBM / L2
constexpr int kSo2LdsArcs = 64;   // arcs staged in LDS; more are read from HBM / L2

template <int NA>
struct So2Shared {
    uint32_t rng_buf[16][64];   // the sampler's window: 64 ChaCha12 blocks = 512 words
    double node[kSo2N];         // the first kSo2N nodes
    double q[64];               // the samples of the current block of 64 iterations ...
    uint64_t pos_after[64];     // ... and the stream position after each of them
    double arc_lo[NA], arc_hi[NA];
};
static_assert(sizeof(So2Shared<kSo2LdsArcs>) <= 40960, "four problems per CU");

// the space as rrt_wave.hpp's motion pass sees it: the arithmetic on 1-wide states, and the arcs wherever they lie
struct So2Checker {
    static constexpr int W = 1;
    const double* lo;
    const double* hi;
    uint32_t na;

    static __device__ __forceinline__ double distance(const double a[1], const double b[1]) { return so2_distance(a[0], b[0]); }
    static __device__ __forceinline__ void interpolate(const double a[1], const double b[1], double t, double out[1]) {
        out[0] = so2_interpolate(a[0], b[0], t);
    }
    __device__ __forceinline__ bool free() const { return na == 0; }
    __device__ __forceinline__ bool state_hit(const double s[1]) const { return so2_arc_hit(lo, hi, na, s[0]); }
};

template <bool LDS_ARCS>
__global__ __launch_bounds__(64) void rrt_so2_kernel(DevParams p) {
    const uint32_t prob = blockIdx.x, lane = threadIdx.x;
    __shared__ So2Shared<LDS_ARCS ? kSo2LdsArcs : 1> sh;
    ProblemState st = p.state[prob];
    if (p.stop_at_goal && st.goal_node >= 0) return;   // already solved: solve() is idempotent
    So2Checker arcs{p.box_lo, p.box_hi, p.n_boxes};
    const uint32_t na = arcs.na;
    if (LDS_ARCS) {   // the checker's table at LDS latency
        for (uint32_t i = lane; i < na; i += 64u) {
            sh.arc_lo[i] = p.box_lo[i];
            sh.arc_hi[i] = p.box_hi[i];
        }
        arcs.lo = sh.arc_lo;
        arcs.hi = sh.arc_hi;
    }
    const size_t cap = p.cap;
    double* tree = p.tree + (size_t)prob * cap;
    int32_t* parent = p.parent + (size_t)prob * cap;
    const double* goal_c = p.goal_c + prob;
    const double target = goal_c[0];
    const double goal_radius = p.goal_thr[prob];   // the radius itself: the goal test compares the SO(2) distance

    uint32_t n = st.n_nodes;
    const uint32_t n_lds0 = n < (uint32_t)kSo2N ? n : (uint32_t)kSo2N;
    for (uint32_t i = lane; i < n_lds0; i += 64u) sh.node[i] = tree[i];   // a solve call continues the tree an earlier one (or set_tree) left in HBM
    RngWindow rng;
    rng.init(sh.rng_buf, p.seed, p.first_problem_id + prob, st.draws);
    __syncthreads();

    int32_t stop = 1;   // OXHIP_STOP_ITERATIONS
    uint64_t h = uni64(st.checksum);
    uint64_t draws = st.draws;   // the stream position after the last iteration that ran (the window itself runs ahead by up to a block)
    uint64_t sampled = 0;        // iterations of this launch whose samples have been drawn
    for (uint64_t it = 0; it < p.budget; ++it) {
        if (!p.freeze && n >= p.max_nodes) { stop = 2; break; }

        // 2. sample (rrt.rs:177-184): random_bool, then the target or random_range(lo..hi); a block of 64 iterations at a time
        if (it >= sampled) {
            const uint32_t m = p.budget - sampled < 64u ? (uint32_t)(p.budget - sampled) : 64u;
            sample_block64<1, false>(rng, p, 1, goal_c, 0.0, m, lane, 0u, [&](uint32_t b, const double (&qs)[1], uint64_t pos_after) {
                sh.q[b] = qs[0];
                sh.pos_after[b] = pos_after;
            });
            sampled += m;
            rrt_wave_publish();
        }
        const uint32_t slot = (uint32_t)it & 63u;
        const double q = sh.q[slot];
        draws = sh.pos_after[slot];

        // 3. nearest neighbour (rrt.rs:187-196): lexicographic (distance, index) minimum; a NaN distance of node 0 keeps node 0
        //    (every later comparison with it fails), a NaN elsewhere never wins
        const uint32_t n_lds = n < (uint32_t)kSo2N ? n : (uint32_t)kSo2N;
        Exact e{__builtin_inf(), 0xFFFFFFFFu};
        double d0 = 0.0;
        for (uint32_t i = lane; i < n_lds; i += 64u) {
            const double d = so2_distance(sh.node[i], q);
            if (i == 0) d0 = d;
            if (d < e.dist) { e.dist = d; e.idx = i; }
        }
        for (uint32_t i = n_lds + lane; i < n; i += 64u) {   // nodes beyond the mirror (indices keep ascending within a lane)
            const double d = so2_distance(tree[i], q);
            if (d < e.dist) { e.dist = d; e.idx = i; }
        }
        e = exact_wave_reduce(e);
        d0 = readlane_f64(d0, 0);
        uint32_t nearest = e.idx;
        double min_dist = e.dist;
        if (d0 != d0 || nearest == 0xFFFFFFFFu) { nearest = 0; min_dist = d0; }
        nearest = uni(nearest);
        const double q_near = nearest < (uint32_t)kSo2N ? sh.node[nearest] : tree[nearest];

        // 4. steer (rrt.rs:199-208)
        double q_new = q;
        if (min_dist > p.max_distance) q_new = so2_interpolate(q_near, q, p.max_distance / min_dist);

        // 5. check_motion (rrt.rs:211 -> :90-116)
        const double q_near1[1] = {q_near}, q_new1[1] = {q_new};
        const bool ok = !rrt_wave_motion_invalid(arcs, q_near1, q_new1, p.res, lane);

        h = chk_push(h, iter_digest<1>(nearest, q_new1, 1, ok));
        st.iterations++;

        bool hit = false;
        if (ok) {
            st.accepted++;
            if (!p.freeze) {
                // 6. insert (rrt.rs:213-217)
                if (lane == 0) {
                    tree[n] = q_new;
                    parent[n] = (int32_t)nearest;
                    if (n < (uint32_t)kSo2N) sh.node[n] = q_new;
                }
                // the next scan is this wave's own and LDS is in order per wave (the fences keep the compiler from moving the store)
                rrt_wave_publish();
                ++n;
                // 7. goal test (rrt.rs:220-223)
                if (so2_distance(q_new, target) <= goal_radius) {
                    if (st.goal_node < 0) st.goal_node = (int32_t)(n - 1);
                    hit = true;
                }
            }
        }
        if (hit && p.stop_at_goal) { stop = 0; break; }
    }
    if (lane == 0) {
        st.checksum = h;
        st.n_nodes = n;
        st.draws = draws;
        st.stop_reason = stop;
        p.state[prob] = st;
    }
}

void launch_rrt_so2(const DevParams& p, hipStream_t stream) {
    const dim3 grid(p.n_problems), block(64);
    if (p.n_boxes <= (uint32_t)kSo2LdsArcs) hipLaunchKernelGGL(rrt_so2_kernel<true>, grid, block, 0, stream, p);
    else hipLaunchKernelGGL(rrt_so2_kernel<false>, grid, block, 0, stream, p);
}

// ---- the checker's stand-alone entry points
__global__ void so2_is_valid_kernel(DevParams p, const double* states, uint32_t n, uint8_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = so2_arc_hit(p.box_lo, p.box_hi, p.n_boxes, states[i]) ? 0 : 1;
}
void launch_so2_is_valid(const DevParams& p, const double* states, uint32_t n, uint8_t* out, hipStream_t s) {
    hipLaunchKernelGGL(so2_is_valid_kernel, dim3((n + 255) / 256), dim3(256), 0, s, p, states, n, out);
}

// one wave per motion
__global__ __launch_bounds__(256) void so2_check_motion_kernel(DevParams p, const double* from, const double* to, uint32_t n,
                                                                uint8_t* out) {
    const uint32_t m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (m >= n) return;
    const double f[1] = {from[m]}, g[1] = {to[m]};
    const bool any = rrt_wave_motion_invalid(So2Checker{p.box_lo, p.box_hi, p.n_boxes}, f, g, p.res, lane);   // the planner's own
    if (lane == 0) out[m] = any ? 0 : 1;
}
void launch_so2_check_motion(const DevParams& p, const double* from, const double* to, uint32_t n, uint8_t* out, hipStream_t s) {
    hipLaunchKernelGGL(so2_check_motion_kernel, dim3((n + 3) / 4), dim3(256), 0, s, p, from, to, n, out);
}

}  // namespace oxhip
