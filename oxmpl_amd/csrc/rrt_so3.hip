// rrt_so3.hip -- RRT (oxmpl/src/geometric/planners/rrt.rs:170-225) over SO3StateSpace (unit quaternions,
// oxmpl/src/base/spaces/so3_state_space.rs) with the forbidden-cone checker of the reference's SO(3) fixture
// (oxmpl/tests/rrt_so3ss_tests.rs:46-56).  Arithmetic: so3_device.hpp.
//
// ONE WAVE PER PROBLEM (a 64-thread workgroup, four per CU -- the shape of rrt_connect.hip / rrt_connect_se2.hip): an
// iteration is a chain of dependent steps, so what counts is the length of that chain.  The tree lives in HBM as SoA
// [4][cap] (every store lands there) and its first kSo3N nodes are mirrored in LDS; the cones are staged in LDS when they
// fit.  Per iteration:
//   sample    lane j evaluates rejection attempt j of sample_uniform (so3_state_space.rs:201-231) -- words 1 + 4j .. 4j + 4
//             after the Bernoulli word -- and a ballot takes the first accepted attempt (so3_sample below)
//   nearest   each lane computes the exact distance (acos included) of its strided nodes, strict '<' in ascending index
//             order, then the wave's lexicographic (distance, index) minimum: the reference's argmin with the lowest index
//             among ties.  No binary32 screen: the distance is not a norm, and parity needs none.
//   steer     interpolate(q_near, q_rand, max_distance / min_dist) when min_dist > max_distance  (rrt.rs:199-208)
//   motion    the interpolated states of check_motion (rrt.rs:90-116) are dealt to the lanes, 64 per pass
//   insert    lane 0 stores node n (HBM + LDS mirror), then the goal test distance(q_new, target) <= radius
// The checksum is the per-iteration polynomial of ABI 2 (rrt_device.hpp, iter_digest) over the four coordinates.
// The wave-local fence and the motion pass are rrt_wave.hpp's, shared with rrt_so2.hip.
#include "oxhip_internal.hpp"
#include "rrt_device.hpp"
#include "so3_device.hpp"
#include "so3_sampler.hpp"
#include "rrt_wave.hpp"

namespace oxhip {

constexpr int kSo3N = 1024;        // tree nodes mirrored in LDS (32 B each); beyond that nodes are read from HBM / L2
constexpr int kSo3LdsCones = 32;   // cones staged in LDS; more are read from HBM / L2

template <int NC>
struct So3Shared {
    uint32_t rng_buf[16][64];   // the sampler's window: 64 ChaCha12 blocks = 512 words
    double4 node[kSo3N];        // (x, y, z, w) of the first kSo3N nodes
    double cone_c[4][NC];       // cone centres, SoA (the layout of DevParams::sph_c)
    double cone_r[NC];          // cone radii as given
};
static_assert(sizeof(So3Shared<kSo3LdsCones>) <= 40960, "four problems per CU");

// rrt.rs:177-184 with SO3StateSpace::sample_uniform (so3_sampler.hpp: 64 rejection attempts side by side) and the ball goal's
// sample_goal (the target, no draw).  Wave-uniform result.
__device__ __forceinline__ void so3_sample(RngWindow& rng, const DevParams& p, const double target[4], uint32_t lane, double q[4]) {
    bool goal;
    if (p.p_int == ~0ull) goal = true;              // Bernoulli ALWAYS_TRUE: no draw
    else goal = rng.next<false>() < p.p_int;        // one u64
    if (goal) {
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = target[k];
        return;
    }
    so3_sample_uniform_wave(rng, p, lane, q);
}

// the space as rrt_wave.hpp's motion pass sees it: the arithmetic on quaternions, and the cones wherever they lie
struct So3Checker {
    static constexpr int W = 4;
    const double* cc;    // centres, SoA [4][stride]
    const double* cr;    // radii as given
    uint32_t stride, nc;

    static __device__ __forceinline__ double distance(const double a[4], const double b[4]) { return so3_distance(a, b); }
    static __device__ __forceinline__ void interpolate(const double a[4], const double b[4], double t, double out[4]) {
        so3_interpolate(a, b, t, out);
    }
    __device__ __forceinline__ bool free() const { return nc == 0; }
    __device__ __forceinline__ bool state_hit(const double s[4]) const { return so3_cone_hit(cc, stride, cr, nc, s); }
};

template <bool LDS_CONES>
__global__ __launch_bounds__(64) void rrt_so3_kernel(DevParams p) {
    const uint32_t prob = blockIdx.x, lane = threadIdx.x;
    __shared__ So3Shared<LDS_CONES ? kSo3LdsCones : 1> sh;
    ProblemState st = p.state[prob];
    if (p.stop_at_goal && st.goal_node >= 0) return;   // already solved: solve() is idempotent
    So3Checker cones{p.sph_c, p.sph_r, p.n_spheres, p.n_spheres};
    const uint32_t nc = cones.nc;
    if (LDS_CONES) {   // the checker's table at LDS latency
        for (uint32_t i = lane; i < nc; i += 64u) {
#pragma unroll
            for (int k = 0; k < 4; ++k) sh.cone_c[k][i] = p.sph_c[(size_t)k * nc + i];
            sh.cone_r[i] = p.sph_r[i];
        }
        cones.cc = &sh.cone_c[0][0];
        cones.cr = sh.cone_r;
        cones.stride = (uint32_t)kSo3LdsCones;
    }
    const size_t cap = p.cap;
    double* tree = p.tree + (size_t)prob * 4 * cap;
    int32_t* parent = p.parent + (size_t)prob * cap;
    const double target[4] = {p.goal_c[(size_t)prob * 4], p.goal_c[(size_t)prob * 4 + 1], p.goal_c[(size_t)prob * 4 + 2],
                              p.goal_c[(size_t)prob * 4 + 3]};
    const double goal_radius = p.goal_thr[prob];   // the radius itself: the goal test compares the SO(3) distance

    uint32_t n = st.n_nodes;
    const uint32_t n_lds0 = n < (uint32_t)kSo3N ? n : (uint32_t)kSo3N;
    for (uint32_t i = lane; i < n_lds0; i += 64u)   // a solve call continues the tree an earlier one (or set_tree) left in HBM
        sh.node[i] = make_double4(tree[i], tree[cap + i], tree[2 * cap + i], tree[3 * cap + i]);
    RngWindow rng;
    rng.init(sh.rng_buf, p.seed, p.first_problem_id + prob, st.draws);
    __syncthreads();

    int32_t stop = 1;   // OXHIP_STOP_ITERATIONS
    uint64_t h = uni64(st.checksum);
    for (uint64_t it = 0; it < p.budget; ++it) {
        if (!p.freeze && n >= p.max_nodes) { stop = 2; break; }

        // 2. sample (rrt.rs:177-184)
        double q[4];
        so3_sample(rng, p, target, lane, q);

        // 3. nearest neighbour (rrt.rs:187-196): lexicographic (distance, index) minimum; a NaN distance of node 0 keeps node 0
        //    (every later comparison with it fails), a NaN elsewhere never wins
        const uint32_t n_lds = n < (uint32_t)kSo3N ? n : (uint32_t)kSo3N;
        Exact e{__builtin_inf(), 0xFFFFFFFFu};
        double d0 = 0.0;
        for (uint32_t i = lane; i < n_lds; i += 64u) {
            const double4 c4 = sh.node[i];
            const double c[4] = {c4.x, c4.y, c4.z, c4.w};
            const double d = so3_distance(c, q);
            if (i == 0) d0 = d;
            if (d < e.dist) { e.dist = d; e.idx = i; }
        }
        for (uint32_t i = n_lds + lane; i < n; i += 64u) {   // nodes beyond the mirror (indices keep ascending within a lane)
            const double c[4] = {tree[i], tree[cap + i], tree[2 * cap + i], tree[3 * cap + i]};
            const double d = so3_distance(c, q);
            if (d < e.dist) { e.dist = d; e.idx = i; }
        }
        e = exact_wave_reduce(e);
        d0 = readlane_f64(d0, 0);
        uint32_t nearest = e.idx;
        double min_dist = e.dist;
        if (d0 != d0 || nearest == 0xFFFFFFFFu) { nearest = 0; min_dist = d0; }
        nearest = uni(nearest);
        double q_near[4];
        if (nearest < (uint32_t)kSo3N) {
            const double4 c4 = sh.node[nearest];
            q_near[0] = c4.x; q_near[1] = c4.y; q_near[2] = c4.z; q_near[3] = c4.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) q_near[k] = tree[(size_t)k * cap + nearest];
        }

        // 4. steer (rrt.rs:199-208)
        double q_new[4];
        if (min_dist > p.max_distance) {
            const double t = p.max_distance / min_dist;
            so3_interpolate(q_near, q, t, q_new);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) q_new[k] = q[k];
        }

        // 5. check_motion (rrt.rs:211 -> :90-116)
        const bool ok = !rrt_wave_motion_invalid(cones, q_near, q_new, p.res, lane);

        h = chk_push(h, iter_digest<4>(nearest, q_new, 4, ok));
        st.iterations++;

        bool hit = false;
        if (ok) {
            st.accepted++;
            if (!p.freeze) {
                // 6. insert (rrt.rs:213-217)
                if (lane == 0) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) tree[(size_t)k * cap + n] = q_new[k];
                    parent[n] = (int32_t)nearest;
                    if (n < (uint32_t)kSo3N) sh.node[n] = make_double4(q_new[0], q_new[1], q_new[2], q_new[3]);
                }
                // the next scan is this wave's own and LDS is in order per wave (the fences keep the compiler from moving the store)
                rrt_wave_publish();
                ++n;
                // 7. goal test (rrt.rs:220-223)
                if (so3_distance(q_new, target) <= goal_radius) {
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
        st.draws = rng.pos;
        st.stop_reason = stop;
        p.state[prob] = st;
    }
}

void launch_rrt_so3(const DevParams& p, hipStream_t stream) {
    const dim3 grid(p.n_problems), block(64);
    if (p.n_spheres <= (uint32_t)kSo3LdsCones) hipLaunchKernelGGL(rrt_so3_kernel<true>, grid, block, 0, stream, p);
    else hipLaunchKernelGGL(rrt_so3_kernel<false>, grid, block, 0, stream, p);
}

// ---- stand-alone primitives (parity tests of the SO(3) arithmetic and of the checker)
__global__ void so3_op_kernel(uint32_t op, const double* a, const double* b, const double* t, uint32_t n, double* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (op == 2) { out[i] = ox_acos(a[i]); return; }
    const double x[4] = {a[4 * (size_t)i], a[4 * (size_t)i + 1], a[4 * (size_t)i + 2], a[4 * (size_t)i + 3]};
    const double y[4] = {b[4 * (size_t)i], b[4 * (size_t)i + 1], b[4 * (size_t)i + 2], b[4 * (size_t)i + 3]};
    if (op == 0) { out[i] = so3_distance(x, y); return; }
    double o[4];
    so3_interpolate(x, y, t[i], o);
#pragma unroll
    for (int k = 0; k < 4; ++k) out[4 * (size_t)i + k] = o[k];
}
void launch_so3_op(uint32_t op, const double* a, const double* b, const double* t, uint32_t n, double* out, hipStream_t s) {
    hipLaunchKernelGGL(so3_op_kernel, dim3((n + 255) / 256), dim3(256), 0, s, op, a, b, t, n, out);
}

__global__ void so3_is_valid_kernel(DevParams p, const double* states, uint32_t n, uint8_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double s[4] = {states[4 * (size_t)i], states[4 * (size_t)i + 1], states[4 * (size_t)i + 2], states[4 * (size_t)i + 3]};
    out[i] = so3_cone_hit(p.sph_c, p.n_spheres, p.sph_r, p.n_spheres, s) ? 0 : 1;
}
void launch_so3_is_valid(const DevParams& p, const double* states, uint32_t n, uint8_t* out, hipStream_t s) {
    hipLaunchKernelGGL(so3_is_valid_kernel, dim3((n + 255) / 256), dim3(256), 0, s, p, states, n, out);
}

// one wave per motion
__global__ __launch_bounds__(256) void so3_check_motion_kernel(DevParams p, const double* from, const double* to, uint32_t n,
                                                                uint8_t* out) {
    const uint32_t m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (m >= n) return;
    const double f[4] = {from[4 * (size_t)m], from[4 * (size_t)m + 1], from[4 * (size_t)m + 2], from[4 * (size_t)m + 3]};
    const double g[4] = {to[4 * (size_t)m], to[4 * (size_t)m + 1], to[4 * (size_t)m + 2], to[4 * (size_t)m + 3]};
    const bool any = rrt_wave_motion_invalid(So3Checker{p.sph_c, p.sph_r, p.n_spheres, p.n_spheres}, f, g, p.res, lane);
    if (lane == 0) out[m] = any ? 0 : 1;
}
void launch_so3_check_motion(const DevParams& p, const double* from, const double* to, uint32_t n, uint8_t* out, hipStream_t s) {
    hipLaunchKernelGGL(so3_check_motion_kernel, dim3((n + 3) / 4), dim3(256), 0, s, p, from, to, n, out);
}

}  // namespace oxhip
