// seq_space.hpp -- the state space as ONE thread sees it: the kernels in which a thread owns a state or a motion of its own (PRM's
// query sets, the re-check, the shortcut's pair matrix and DP -- shortcut_core.hip, one pair of kernels for an RRT batch's paths and a
// PRM batch's --, the shortest paths' weights) are written once over SeqSpace<DIM>.
// DIM = 1..8 is R^DIM, DIM = 0 is SO(3) (unit quaternions among forbidden cones), DIM = -1 is SO(2) (one angle among forbidden
// arcs).  The members forward to motion_seq.hpp / so3_motion_seq.hpp / so3_device.hpp / so2_device.hpp, so every bit is the one
// those functions give.  space_dispatch is the host's way in: R^n or SO(3), and SO(2) for the callers that ask for it.
#pragma once
#include <type_traits>
#include <utility>

#include "rrt_device.hpp"
#include "motion_seq.hpp"
#include "so2_device.hpp"
#include "so3_device.hpp"
#include "so3_motion_seq.hpp"

namespace oxhip {

template <int DIM>
struct SeqSpace {                                  // R^DIM
    static constexpr int W = DIM;                  // components of a state
    using Checker = DevParams;                     // what a kernel takes as its argument
    static Checker checker(const DevParams& p) { return p; }

    static __device__ __forceinline__ void load(const double* row, double out[W]) {
#pragma unroll
        for (int k = 0; k < W; ++k) out[k] = row[k];
    }
    // the bits of oxhip_distance_batch
    static __device__ __forceinline__ double distance(const double a[W], const double b[W]) { return sqrt(dist2<W>(a, b, W)); }
    // distance(s, m) < connection_radius, decided exactly on the squared distance: `near` is its threshold (sqrt_le_threshold)
    static __device__ __forceinline__ bool connects(const double s[W], const double m[W], double near) { return dist2<W>(s, m, W) <= near; }
    // goal.is_satisfied is goal_measure(m, g) <= thr: here the squared distance, against the squared-distance threshold of the
    // radius.  (The comparison stands in the query kernels, which read thr after the measure: prm_kernels.hip.)
    static __device__ __forceinline__ double goal_measure(const double m[W], const double g[W]) { return dist2<W>(m, g, W); }
    static __device__ __forceinline__ bool state_valid(const Checker& p, const double s[W]) { return state_valid_seq<W>(p, s); }
    static __device__ __forceinline__ bool motion_valid(const Checker& p, const double from[W], const double to[W], double filt_abs) {
        return motion_valid_seq<W>(p, from, to, filt_abs);
    }
    static __device__ __forceinline__ bool motion_valid(const Checker& p, const double from[W], const double to[W]) {   // the host's margin
        return motion_valid_seq<W>(p, from, to);
    }
    // the midpoint filter's absolute margin with this motion's ends in play: a state given by the caller may lie outside the bounds
    // (the filter only ever drops spheres that cannot be hit, so the verdict does not depend on the margin)
    static __device__ __forceinline__ double motion_margin(double base, const double from[W], const double to[W]) {
#pragma unroll
        for (int k = 0; k < W; ++k) base = fmax(base, 1e-9 * fmax(fabs(from[k]), fabs(to[k])));
        return base;
    }

    // The obstacle tables are SoA [dim][n], read by the shared device functions at a wave-uniform index: as kernel arguments their
    // per-dimension rows become scalar address pairs and scalar operands, about ten SGPRs per dimension, and from R^6 on that spills
    // SGPRs.  Here the three table pointers pass through a VGPR first, so the same loads are issued as vector loads of the same
    // addresses: the same values, the same arithmetic, no spill.  (The radii, thresholds and the box count follow for R^8's last
    // SGPRs.)  Used by the re-check's kernels (prm_revalidate.hip) only.
    template <typename T>
    static __device__ __forceinline__ void vector_pointer(const T*& ptr) {
        asm volatile("" : "+v"(ptr));
    }
    static __device__ __forceinline__ Checker vgpr_pointers(const Checker& p) {
        Checker q = p;
        vector_pointer(q.sph_c);
        vector_pointer(q.box_lo);
        vector_pointer(q.box_hi);
        vector_pointer(q.sph_r);
        vector_pointer(q.sph_thr);
        asm volatile("" : "+v"(q.n_boxes));   // (and with it the box tables' row strides k * n_boxes)
        return q;
    }
};

template <>
struct SeqSpace<0> {                               // SO(3)
    static constexpr int W = 4;
    using Checker = So3Cones;                      // (the whole DevParams costs SGPRs: so3_motion_seq.hpp)
    static Checker checker(const DevParams& p) { return So3Cones{p.sph_c, p.sph_r, p.n_spheres, p.res}; }

    static __device__ __forceinline__ void load(const double* row, double out[4]) {
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k] = row[k];
    }
    // the bits of oxhip_so3_op_batch op 0
    static __device__ __forceinline__ double distance(const double a[4], const double b[4]) { return so3_distance(a, b); }
    // prm.rs:134 / :251 (strict): `near` is the connection radius itself
    static __device__ __forceinline__ bool connects(const double s[4], const double m[4], double near) { return so3_distance(s, m) < near; }
    // goal.is_satisfied: distance(state, target) <= radius
    static __device__ __forceinline__ double goal_measure(const double m[4], const double g[4]) { return so3_distance(m, g); }
    static __device__ __forceinline__ bool state_valid(const Checker& p, const double s[4]) { return !so3_cone_hit(p.c, p.n, p.r, p.n, s); }
    static __device__ __forceinline__ bool motion_valid(const Checker& p, const double from[4], const double to[4], double = 0.0) {   // no filter
        return so3_motion_valid_seq(p.c, p.n, p.r, p.n, from, to, p.res);
    }
    static __device__ __forceinline__ double motion_margin(double base, const double*, const double*) { return base; }
    static __device__ __forceinline__ Checker vgpr_pointers(const Checker& p) { return p; }   // (four scalars: nothing spills)
};

template <>
struct SeqSpace<-1> {                              // SO(2)
    static constexpr int W = 1;
    using Checker = So2Arcs;
    static Checker checker(const DevParams& p) { return So2Arcs{p.box_lo, p.box_hi, p.n_boxes, p.res}; }

    static __device__ __forceinline__ void load(const double* row, double out[1]) { out[0] = row[0]; }
    static __device__ __forceinline__ double distance(const double a[1], const double b[1]) { return so2_distance(a[0], b[0]); }
    static __device__ __forceinline__ bool connects(const double s[1], const double m[1], double near) { return so2_distance(s[0], m[0]) < near; }
    // goal.is_satisfied: distance(state, target) <= radius
    static __device__ __forceinline__ double goal_measure(const double m[1], const double g[1]) { return so2_distance(m[0], g[0]); }
    static __device__ __forceinline__ bool state_valid(const Checker& p, const double s[1]) { return !so2_arc_hit(p.lo, p.hi, p.n, s[0]); }
    static __device__ __forceinline__ bool motion_valid(const Checker& p, const double from[1], const double to[1], double = 0.0) {   // no filter
        return so2_motion_valid_seq(p.lo, p.hi, p.n, from[0], to[0], p.res);
    }
    static __device__ __forceinline__ double motion_margin(double base, const double*, const double*) { return base; }
    static __device__ __forceinline__ Checker vgpr_pointers(const Checker& p) { return p; }   // (four scalars: nothing spills)
};

// The host's way to an instantiation: f(std::integral_constant<int, D>{}) with D = dim in LO..8 (a caller that never sees R^1
// passes LO = 2) -- for kernels that exist over R^n only -- and space_dispatch below it, which takes the oxhip_space_kind: D = 0
// for SO(3) and, for a caller that opts in with SO2 = true, D = -1 for SO(2).  Without the opt-in nothing is instantiated over
// SO(2): the PRM files do not ask (no roadmap is built over SO(2)), the RRT re-check and the shortcut's RRT entry do.
template <int LO = 1, typename F>
void dim_dispatch(uint32_t dim, F&& f) {
    if constexpr (LO <= 1)
        if (dim == 1) return f(std::integral_constant<int, 1>{});
    switch (dim) {
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 5: f(std::integral_constant<int, 5>{}); break;
        case 6: f(std::integral_constant<int, 6>{}); break;
        case 7: f(std::integral_constant<int, 7>{}); break;
        default: f(std::integral_constant<int, 8>{}); break;
    }
}
template <int LO = 1, bool SO2 = false, typename F>
void space_dispatch(uint32_t space, uint32_t dim, F&& f) {
    if (space == OXHIP_SPACE_SO3) return f(std::integral_constant<int, 0>{});
    if constexpr (SO2)
        if (space == OXHIP_SPACE_SO2) return f(std::integral_constant<int, -1>{});
    dim_dispatch<LO>(dim, std::forward<F>(f));
}
// the PRM launchers' `bool so3` as a space kind
constexpr uint32_t prm_space(bool so3) { return so3 ? OXHIP_SPACE_SO3 : OXHIP_SPACE_REAL_VECTOR; }

}  // namespace oxhip
