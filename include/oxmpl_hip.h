/*
 * oxmpl_hip.h -- C ABI of liboxmpl_hip.so: the MI355X (gfx950) batched RRT hot path.
 *
 * The reference (rossng/oxmpl, Rust) has no C ABI; the boundary of this path is the
 * trait `Planner<S, SP, G>` (oxmpl/src/base/planner.rs:26-60) over `StateSpace`
 * (space.rs:78-145), `StateValidityChecker` (validity.rs:39-48) and `Goal*`
 * (goal.rs:12-41).  The entry points below are what a Rust `extern "C"` block (or
 * cgo / ctypes) binds to put the HIP path behind those traits; each cites the
 * reference item it replaces.  INTEGRATION.md shows the Rust-side binding.
 *
 * Conventions: plain pointers + sizes, caller owns every host array (copied during
 * the call), all states are f64, AoS `[n][dim]` on this boundary (SoA on the device).
 * Every function returns an oxhip_status; nothing aborts or throws across the ABI.
 * A handle is bound to one HIP device and one stream and is not re-entrant;
 * different handles may be driven from different host threads / processes.
 */
#ifndef OXMPL_HIP_H
#define OXMPL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: get_stamps takes a capacity (ABI 1 wrote 32, later 64 words unasked); kernel kinds 3 / 4 retired; the per-iteration checksum is
 *    the polynomial H <- H P + g (ABI 1 as first shipped chained FNV-1a); oxhip_rrt_config gained goal_sampler / debug_flags */
#define OXHIP_ABI_VERSION 2
#define OXHIP_MAX_DIM 8

/* Status codes.  0-5 mirror `PlanningError` (oxmpl/src/base/error.rs:97-108) in
 * declaration order (+1); 16-18 mirror the sampling/space errors the reference
 * would panic on via unwrap() (rrt.rs:180,183; real_vector_state_space.rs:239-244,
 * 78-83); 32+ are HIP/runtime conditions that have no reference counterpart. */
typedef enum oxhip_status {
    OXHIP_OK = 0,                       /* Ok(Path) / success */
    OXHIP_ERR_TIMEOUT = 1,              /* PlanningError::Timeout            rrt.rs:172-174 */
    OXHIP_ERR_NO_SOLUTION_FOUND = 2,    /* PlanningError::NoSolutionFound    rrt.rs:226 (iteration / node cap) */
    OXHIP_ERR_PLANNER_UNINITIALISED = 3,/* PlanningError::PlannerUninitialised rrt.rs:160-163 */
    OXHIP_ERR_INVALID_START_STATE = 4,  /* PlanningError::InvalidStartState  (unused by RRT, kept for parity of the enum) */
    OXHIP_ERR_UNSAMPLED_STATE_SPACE = 5,/* PlanningError::UnsampledStateSpace (PRM only) */
    OXHIP_ERR_BAD_ARG = 16,             /* null pointer, dim out of range, goal_bias outside [0,1], ... */
    OXHIP_ERR_UNBOUNDED = 17,           /* StateSamplingError::UnboundedDimension  rvss.rs:239-241 */
    OXHIP_ERR_ZERO_VOLUME = 18,         /* StateSamplingError::ZeroVolume / StateSpaceError::InvalidBound */
    OXHIP_ERR_CAPACITY = 19,            /* caller buffer too small; required length is still written */
    OXHIP_ERR_HIP = 32,                 /* a HIP runtime call failed; see oxhip_last_error_string() */
    OXHIP_ERR_NO_DEVICE = 33            /* no gfx950 device visible -- there is NO CPU fallback */
} oxhip_status;

/* why a problem stopped (per-problem, next to its status) */
typedef enum oxhip_stop_reason {
    OXHIP_STOP_NONE = -1,
    OXHIP_STOP_GOAL = 0,        /* goal.is_satisfied(q_new) with stop_at_goal      rrt.rs:220-223 */
    OXHIP_STOP_ITERATIONS = 1,  /* iteration budget of this solve call exhausted */
    OXHIP_STOP_NODES = 2,       /* tree reached max_nodes */
    OXHIP_STOP_TIMEOUT = 3,     /* wall-clock timeout between kernel chunks */
    OXHIP_STOP_INTERNAL = 4     /* kernel-internal hand-off never completed (bug guard); solve returns OXHIP_ERR_HIP */
} oxhip_stop_reason;

typedef enum oxhip_planner_kind {
    OXHIP_PLANNER_RRT = 0,         /* geometric::RRT         oxmpl/src/geometric/planners/rrt.rs */
    OXHIP_PLANNER_RRT_CONNECT = 1, /* geometric::RRTConnect  oxmpl/src/geometric/planners/rrt_connect.rs (stream kernel only) */
    OXHIP_PLANNER_RRT_STAR = 2     /* geometric::RRTStar     oxmpl/src/geometric/planners/rrt_star.rs.  kernel = OXHIP_KERNEL_AUTO /
                                      OXHIP_KERNEL_LANES: the decoupled design (the node positions of an RRT* run are RRT's, so the
                                      lane-per-query kernel grows the tree and rrt_star_wire.hip then chooses parents and rewires:
                                      R^2 .. R^6, trees that fit the register rows); OXHIP_KERNEL_STREAM: rrt_star.hip, everything
                                      in one kernel (any dimension <= 8, any size).  Same results bit for bit. */
} oxhip_planner_kind;

/* State space of a batch.  oxmpl has RealVectorStateSpace, SO2StateSpace and SO3StateSpace; SE(2) is not in the
 * reference (docs/BACKLOG.md:12-14) and is assembled here from the first two (see rrt_connect_se2.hip):
 * state (x, y, theta), distance = 1.0 * d_xy + 0.5 * d_theta, extent = extent_xy + 0.5 * PI.
 * SO(3) is SO3StateSpace itself (rrt_so3.hip): states are quaternions (x, y, z, w) -- normalising them is the caller's job, as
 * in the reference -- and the config's bounds are REINTERPRETED: bounds[0..3] = the centre quaternion, bounds[4] = max_angle
 * (so3_state_space.rs:57-76: negative = OXHIP_ERR_ZERO_VOLUME, the mirror of StateSpaceError; clamped to PI; NaN reads as PI,
 * as f64::min has it; the unbounded space is centre (0, 0, 0, 1) and max_angle PI); bounds[5..] are ignored.
 * distance = abs_dot > 1 - 1e-9 ? 0 : acos(abs_dot); interpolate = LERP + normalise above |dot| 0.9995, else SLERP; extent
 * 0.5 * PI.  acos / sin are the portable routines ox_acos / ox_sincos (below one ulp; the CPU test suite restates them), so
 * against a rustc-built oxmpl (libm) a run is within a few ulp per evaluation, not bit-exact: PARITY UNPINNED.
 * Validity: oxhip_rrt_batch_set_spheres with 4-wide centres, read as cones in the SO(3) metric -- a state is valid iff
 * distance(centre, q) > radius for every cone (strict; the ForbiddenConeChecker of oxmpl/tests/rrt_so3ss_tests.rs:46-56).
 *
 * SE(3) = R^3 x SO(3) is not in the reference either (docs/BACKLOG.md:12-14); it is assembled from the reference's
 * RealVectorStateSpace and SO3StateSpace the way SE(2) was, with OMPL's SE(3) weights (rrt_connect_se3.hip).  Every operation is
 * unfused binary64 in the order written here:
 *   state        dim = 7: (x, y, z, qx, qy, qz, qw), AoS; normalising the quaternion is the caller's job, as for SO(3)
 *   bounds       bounds[0..5] = (lo, hi) of x, y, z, validated as RealVectorStateSpace::new(3, ..) (OXHIP_ERR_UNBOUNDED,
 *                OXHIP_ERR_ZERO_VOLUME); bounds[6..9] = the rotation's centre quaternion, bounds[10] = max_angle, read exactly as
 *                an SO(3) batch reads bounds[0..4]; bounds[11..15] are ignored
 *   distance     1.0 * distance_R3(xyz) + 1.0 * distance_SO3(q): the two component distances, then one add
 *   interpolate  xyz: from + (to - from) * t; q: SO(3)'s interpolate; the same t
 *   sample       x, y, z in that order by random_range(lo..hi), then SO(3)'s rejection sampler (four random_range(-1.0..1.0)
 *                words per attempt)
 *   extent       extent_R3 + 0.5 * PI; lvsl = extent * fraction; check_motion steps of lvsl * 0.1 (more than 1e6 validity
 *                checks per edge are refused)
 *   goal         distance(s, target) <= radius; sample_goal = the target (OXHIP_GOAL_SAMPLE_CENTRE, no draw)
 *   validity     a rigid body of B spheres (c_b, r_b) given in the body frame (oxhip_rrt_batch_set_body; default: one sphere of
 *                radius 0 at the origin, a point) among N world spheres (o_j, r_j) (oxhip_rrt_batch_set_spheres, 3-wide centres).
 *                Body sphere b sits at p = rot(q, c_b) + (x, y, z); the state is valid iff sqrt(|p - o_j|^2) > r_b + r_j for
 *                every pair (strict; |.|^2 summed x, y, z in order; r_b + r_j is one add).  Bounds are not part of validity.
 *   rot(q, v)    u = (qx, qy, qz), w = qw:  t = 2 * (u x v);  rot = (v + w * t) + (u x t), component by component, every
 *                cross product component evaluated as a*b - c*d:  (u x v)_x = uy*vz - uz*vy, _y = uz*vx - ux*vz, _z = ux*vy - uy*vx
 *   planner      RRTConnect (rrt_connect.rs:86-309) as for the other RRTConnect rows; PARITY UNPINNED (nothing to compare with). */
typedef enum oxhip_space_kind {
    OXHIP_SPACE_REAL_VECTOR = 0,  /* RealVectorStateSpace(dim)  oxmpl/src/base/spaces/real_vector_state_space.rs */
    OXHIP_SPACE_SE2 = 1,          /* R^2 x SO(2): dim must be 3, bounds = (x), (y), (theta: clamped to [-PI, PI]);
                                     planner must be OXHIP_PLANNER_RRT_CONNECT; validity = oxhip_rrt_batch_set_segments */
    OXHIP_SPACE_SO3 = 2,          /* SO3StateSpace  oxmpl/src/base/spaces/so3_state_space.rs: dim must be 4, bounds as above.
                                     RRT batches: planner must be OXHIP_PLANNER_RRT with kernel OXHIP_KERNEL_AUTO or OXHIP_KERNEL_STREAM
                                     (both run rrt_so3.hip); goal = ball in the SO(3) distance, sample_goal = OXHIP_GOAL_SAMPLE_CENTRE;
                                     validity = cones (oxhip_rrt_batch_set_spheres; set_boxes is OXHIP_ERR_BAD_ARG).
                                     PRM (oxhip_prm_config.space, prm_so3.hip): radius rule only (knn_k must be 0); cones by
                                     oxhip_prm_set_spheres (set_boxes is OXHIP_ERR_BAD_ARG); goal = ball in the SO(3) distance */
    OXHIP_SPACE_SE3 = 3,          /* R^3 x SO(3), see above: dim must be 7; planner must be OXHIP_PLANNER_RRT_CONNECT with kernel
                                     OXHIP_KERNEL_AUTO or OXHIP_KERNEL_STREAM (both run rrt_connect_se3.hip); goal sampler CENTRE;
                                     validity = oxhip_rrt_batch_set_body + oxhip_rrt_batch_set_spheres (set_boxes and
                                     set_segments are OXHIP_ERR_BAD_ARG).  Not a PRM space. */
    OXHIP_SPACE_SO2 = 16          /* SO2StateSpace  oxmpl/src/base/spaces/so2_state_space.rs (rrt_so2.hip): dim
                                     must be 1, one angle per state.  bounds[0..1] = (lo, hi): !(lo < hi) is OXHIP_ERR_ZERO_VOLUME -- the
                                     reference's InvalidBound for lo >= hi, and a NaN bound is refused the same way, as the SE(2)
                                     heading's is; clamped to [-PI, PI] (the full circle is (-PI, PI)); bounds[2..] are ignored.
                                     States are taken as given: starts, goal centres and planted trees are NOT normalised
                                     (SO2State::new normalises, a struct literal does not; the caller chooses).
                                     distance = |rem_euclid(a - b + PI, 2 PI) - PI|; interpolate = the shortest way round on the
                                     normalised ends, from + diff * t on the un-normalised `from`, then normalise; sample =
                                     random_range(lo..hi); extent PI, lvsl = PI * fraction, check_motion steps of lvsl * 0.1 (more than
                                     1e6 validity checks per edge are refused).  Add, subtract, multiply, divide and fmod only: apart
                                     from the RNG stream a run is bit-identical to the reference.
                                     Planner must be OXHIP_PLANNER_RRT with kernel OXHIP_KERNEL_AUTO or OXHIP_KERNEL_STREAM (both run
                                     rrt_so2.hip); goal = distance(s, target) <= radius, sample_goal = OXHIP_GOAL_SAMPLE_CENTRE.
                                     Validity = forbidden arcs: oxhip_rrt_batch_set_boxes with 1-wide rows (min, max), any number; a
                                     state is valid iff its normalised value lies in no closed arc [min, max] (the
                                     ForbiddenAngleChecker of oxmpl/tests/rrt_so2ss_tests.rs).  set_spheres, set_segments and set_body
                                     are OXHIP_ERR_BAD_ARG.  Not a PRM space.  (The values 4 .. 15 stay unknown space kinds.) */
} oxhip_space_kind;

/* GoalSampleableRegion::sample_goal of the ball goal (goal.rs:35-41; the trait leaves the distribution to the implementor).
 * CENTRE: the ball's centre, no RNG word consumed -- README.md:160-162, oxmpl-js/examples/simple_2d_planning.js:30-33.
 * UNIFORM_DISC: the sampler of the reference's own test fixtures, oxmpl/tests/rrt_rvss_tests.rs:55-66 (dim must be 2):
 *   angle  = rng.random_range(0.0..2.0 * PI)      -- one u64 (52-bit transform)
 *   radius = self.radius * rng.random::<f64>().sqrt()   -- one u64 (53 bits x 2^-53)
 *   (x, y) = (cx + radius * angle.cos(), cy + radius * angle.sin())
 * cos / sin are evaluated by the portable routine ox_sincos (oxmpl_amd/csrc/ox_sincos.hpp: Cody-Waite reduction + fdlibm
 * kernels in unfused binary64; the test suite's CPU checker restates it operation for operation).  It differs from glibc's
 * sin / cos by at most one ulp on [0, 2 PI) (the CPU test suite measures how often), so against a rustc-built oxmpl
 * this mode is within north_star's 1e-6 relative bound rather than bit-exact. */
typedef enum oxhip_goal_sampler {
    OXHIP_GOAL_SAMPLE_CENTRE = 0,
    OXHIP_GOAL_SAMPLE_UNIFORM_DISC = 1
} oxhip_goal_sampler;

/* oxhip_rrt_config.debug_flags (tests only; every switch leaves every result bit-identical).  rrt_cells.hip honours
 * OXHIP_DEBUG_ALL_WHOLE_TREE and OXHIP_DEBUG_ONE_LANE_ROUNDS; it has no pair pass, no end-state audit and no memo expiry
 * (its memo lasts while the tree has not grown), so it ignores PAIR_TO_WHOLE_TREE and AUDIT, and SHORT_MEMO in a growing
 * launch; in a frozen launch, where no insert could ever expire the memo, SHORT_MEMO keeps no memo at all. */
typedef enum oxhip_debug_flag {
    OXHIP_DEBUG_PAIR_TO_WHOLE_TREE = 1,   /* rrt_lanes.hip: two-lane near-ties take the whole-tree path like three-way ones */
    OXHIP_DEBUG_AUDIT = 2,                /* rrt_lanes.hip, stamped build: count accepted motions whose end state is invalid (stamps[50]) */
    OXHIP_DEBUG_ALL_WHOLE_TREE = 4,       /* rrt_lanes.hip, rrt_cells.hip: no screen verdict is trusted -- every query that is not answered from the memoized
                                             whole-tree answer takes the whole-tree path (with goal_bias > 0 the memo is then hit constantly) */
    OXHIP_DEBUG_ONE_LANE_ROUNDS = 8,      /* rrt_lanes.hip, rrt_cells.hip: a round commits one lane; the others are re-resolved against the grown tree */
    OXHIP_DEBUG_SHORT_MEMO = 16,          /* rrt_lanes.hip: the memoized answer expires after 8 inserts instead of (ring - 64); rrt_cells.hip, frozen launches:
                                             no answer is memoized (every repeat of an ambiguous query is settled afresh) */
    OXHIP_DEBUG_STAR_TWO_PASS = 32,       /* rrt_star_wire.hip: neighbour lists by a second search instead of the counting pass's chunks */
    OXHIP_DEBUG_STAR_ONE_SEGMENT = 64,    /* rrt_star_wire.hip: one edge-check segment, no overlap with the wiring stream */
    OXHIP_DEBUG_SE2_NO_SEGMENT_GRID = 128,/* rrt_connect_se2.hip / rrt_connect.hip: every interpolated state is tested against every segment / sphere (no grid lookup) */
    OXHIP_DEBUG_SE2_SMALL_LDS = 256,      /* rrt_connect_se2.hip: the shape for batches larger than the chip (512-node shadows, segments from HBM / L2) whatever the batch size */
    OXHIP_DEBUG_SO3_SERIAL_SAMPLER = 512, /* rrt_so3.hip, rrt_connect_se3.hip: sample_uniform attempt by attempt on one lane instead of 64 attempts side by side */
    OXHIP_DEBUG_SE3_BRANCHY_SWEEP = 1024, /* rrt_connect_se3.hip: the motion check decides every (body sphere, obstacle) pair as it meets it (the first kernel's sweep)
                                             instead of sweeping without a branch and deciding only the pairs it could not clear */
    OXHIP_DEBUG_CELLS_NO_PACING = 2048    /* rrt_cells.hip, frozen launches: the waves report their progress to the board as always, but none changes its
                                             issue priority by it (every wave stays at priority 0) */
} oxhip_debug_flag;

typedef enum oxhip_kernel_kind {
    OXHIP_KERNEL_AUTO = 0,      /* RRT (and the geometry of the decoupled RRT*): OXHIP_KERNEL_CELLS in R^2 / R^3 (trees up to 64,512
                                   nodes; any batch size); OXHIP_KERNEL_LANES in R^4 .. R^6 when the tree fits its register rows;
                                   else streaming */
    OXHIP_KERNEL_STREAM = 1,    /* tree streamed from HBM/L2 SoA arrays every iteration: any dimension <= 8, any tree size */
    OXHIP_KERNEL_RESIDENT = 2,  /* tree held in the workgroup's vector registers as binary64, every node scanned in binary64
                                   (R^2 / R^3, <= 10,240 nodes): no binary32 anywhere -- the cross-check of the screened kernels */
    OXHIP_KERNEL_RETIRED_3 = 3, /* (ABI 1: box-pruned resident scan, an experiment) -- OXHIP_ERR_BAD_ARG since ABI 2 */
    OXHIP_KERNEL_RETIRED_4 = 4, /* (ABI 1: binary32 screen + lane-group resolver, round 1's default) -- OXHIP_ERR_BAD_ARG since ABI 2 */
    OXHIP_KERNEL_LANES = 5,     /* resident + binary32 screen with a lane-per-query resolver: up to 64 iterations are
                                   resolved side by side and committed as the longest prefix that keeps the reference's
                                   sequential semantics (rrt_lanes.hip); same results bit for bit */
    OXHIP_KERNEL_CELLS = 6      /* one WAVE per problem; nearest neighbour through an exact grid of cells (per-cell node lists in
                                   HBM / L2, the 3^D cells around a query first, further shells when they cannot rule out the rest),
                                   lane-per-query as above (rrt_cells.hip; R^2 / R^3, any tree size); same results bit for bit */
} oxhip_kernel_kind;

/* RRT::new(max_distance, goal_bias) (rrt.rs:75-83) + RealVectorStateSpace::new(dim, bounds)
 * (real_vector_state_space.rs:65-100) + the termination the reference lacks (rrt.rs:226). */
typedef struct oxhip_rrt_config {
    uint32_t struct_size;               /* = sizeof(oxhip_rrt_config) */
    uint32_t dim;                       /* RealVectorStateSpace::dimension, 1..OXHIP_MAX_DIM */
    double   bounds[2 * OXHIP_MAX_DIM]; /* (lo,hi) pairs, real_vector_state_space.rs:19 */
    double   max_distance;              /* RRT::max_distance  rrt.rs:55 */
    double   goal_bias;                 /* RRT::goal_bias     rrt.rs:57, must be in [0,1] */
    double   lvs_fraction;              /* longest_valid_segment_fraction, default 0.05 (rvss.rs:98);
                                           clamped like set_longest_valid_segment_fraction (rvss.rs:121-129) */
    uint32_t n_problems;                /* independent planner instances in this batch */
    uint32_t max_nodes;                 /* tree capacity per problem (build-defined node cap) */
    uint32_t stop_at_goal;              /* 1: stop a problem at its first goal node (reference behaviour) */
    uint32_t kernel;                    /* oxhip_kernel_kind */
    uint64_t seed;                      /* RNG key: ChaCha12 key = LE(seed)||0^24, stream id = first_problem_id + p */
    uint64_t first_problem_id;          /* global id of problem 0 of this batch (problem-parallel sharding) */
    int32_t  device;                    /* HIP device ordinal */
    uint32_t planner;                   /* oxhip_planner_kind: 0 = RRT (rrt.rs), 1 = RRTConnect (rrt_connect.rs), 2 = RRT* */
    double   search_radius;             /* RRTStar::search_radius (rrt_star.rs:45): neighbours are the nodes with
                                           distance < search_radius (strict); ignored by the other planners */
    uint32_t space;                     /* oxhip_space_kind */
    uint32_t goal_sampler;              /* oxhip_goal_sampler: what GoalSampleableRegion::sample_goal (goal.rs:35-41) draws */
    uint32_t debug_flags;               /* oxhip_debug_flag bits: test-only switches that force rarely taken code paths; results are
                                           identical by construction.  0 in production (the library reads no environment variable) */
    uint32_t star_pool_share;           /* RRT*, decoupled design: neighbour-list pool entries per problem (16 B each, + 4.5 B of chunk
                                           store); 0 = default: 64 x tree capacity, bounded so that the whole batch stays below 24 GB.
                                           The size bounds memory, never results: lists that do not fit are wired in further rounds */
    uint32_t frozen_split;              /* OXHIP_KERNEL_CELLS, solve(freeze = 1): waves a problem's frozen iterations are divided over
                                           (1 .. 64; 0 = automatic).  Results do not depend on it */
    uint32_t reserved;                  /* 0 */
} oxhip_rrt_config;

typedef struct oxhip_rrt_batch oxhip_rrt_batch;

/* ---- library ---- */
int32_t     oxhip_abi_version(void);
const char* oxhip_status_string(int32_t status);
const char* oxhip_last_error_string(void);              /* thread-local detail of the last OXHIP_ERR_* */
int32_t     oxhip_device_count(int32_t* count);         /* OXHIP_ERR_NO_DEVICE when none */

/* ---- batched planner: replaces RRT::new / Planner::setup / Planner::solve ---- */

/* RRT::new + RealVectorStateSpace::new for n_problems instances; allocates device trees. */
int32_t oxhip_rrt_batch_create(const oxhip_rrt_config* cfg, oxhip_rrt_batch** out);
int32_t oxhip_rrt_batch_destroy(oxhip_rrt_batch* b);

/* Device-describable StateValidityChecker (validity.rs:39-48), shared by all problems:
 * a state is valid iff for every sphere distance(centre, p) > radius  (strict, the shape of
 * README.md:147-150) and it is inside no box: NOT(lo_k <= p_k <= hi_k for all k)
 * (the wall of oxmpl/tests/rrt_rvss_tests.rs:24-36).  Replaces any earlier field. */
int32_t oxhip_rrt_batch_set_spheres(oxhip_rrt_batch* b, const double* centres /*[n][dim]*/,
                                    const double* radii /*[n]*/, uint32_t n);
/* (OXHIP_SPACE_SO2: set_boxes takes the forbidden arcs, 1-wide rows: lo[j] = an arc's minimum, hi[j] = its maximum.) */
int32_t oxhip_rrt_batch_set_boxes(oxhip_rrt_batch* b, const double* lo /*[n][dim]*/,
                                  const double* hi /*[n][dim]*/, uint32_t n);

/* SE(2) batches only.  The checker of BASELINE.json configs[3]: a disc robot of radius `clearance` among n line
 * segments (ax, ay, bx, by) -- a state is valid iff its (x, y) is farther than `clearance` from every segment
 * (strict; the heading does not enter).  Replaces any earlier segment set.  Also files the segments in a 256 x 256 lookup grid
 * over the (x, y) bounds on the device (1 MiB; rrt_connect_se2.hip, seg_grid_kernel): the planner's motion checks and
 * oxhip_rrt_batch_check_motion test a state against its cell's segments only -- the same verdicts, by construction. */
int32_t oxhip_rrt_batch_set_segments(oxhip_rrt_batch* b, const double* segments /*[n][4]*/, uint32_t n,
                                     double clearance);

/* SE(3) batches only (OXHIP_ERR_BAD_ARG otherwise).  The rigid body: n spheres, 1 <= n <= 16, centres in the body frame and radii
 * (finite, >= 0).  Replaces any earlier body; a new batch has one sphere of radius 0 at the origin.  The obstacles are the world
 * spheres of oxhip_rrt_batch_set_spheres (centres [n][3]). */
int32_t oxhip_rrt_batch_set_body(oxhip_rrt_batch* b, const double* centres /*[n][3]*/, const double* radii /*[n]*/, uint32_t n);

/* Planner::setup (rrt.rs:140-156) for every problem: clears the tree, pushes start_states[0]
 * (validity of the start is NOT checked, as in the reference), resets counters and the RNG
 * stream.  Goal = ball: is_satisfied(s) = distance(s, centre) <= radius
 * (rrt_rvss_tests.rs:45-49); sample_goal() as oxhip_rrt_config.goal_sampler says. */
int32_t oxhip_rrt_batch_setup(oxhip_rrt_batch* b, const double* starts /*[P][dim]*/,
                              const double* goal_centres /*[P][dim]*/, const double* goal_radii /*[P]*/);

/* Warm start: replace problem `problem`'s tree (RRT::tree, rrt.rs:61) by n >= 1 nodes given as AoS
 * states [n][dim] and parent indices (parents[0] = -1).  Allowed after setup(); counters and the RNG
 * stream are left as they are.  Lets a caller continue a tree grown elsewhere (and lets the parity
 * tests plant adversarial trees). */
int32_t oxhip_rrt_batch_set_tree(oxhip_rrt_batch* b, uint32_t problem, const double* states,
                                 const int32_t* parents, uint32_t n_nodes);

/* ---- re-checking the trees against the obstacles as they are now (rrt_revalidate.hip) ----
 * The semantics are this build's own (the reference has no such call).  OXHIP_PLANNER_RRT over OXHIP_SPACE_REAL_VECTOR (every
 * dimension, spheres and boxes), OXHIP_SPACE_SO3 (cones) and OXHIP_SPACE_SO2 (arcs), every kernel kind.  For every problem,
 * against the batch's current spheres / boxes / cones / arcs (the midpoint filter and the sphere grid are refreshed first, as solve does):
 *   edge_ok[i], i >= 1, is the verdict of the batch's own check_motion(from = node parent[i], to = node i) -- the direction the
 *     planner checked the edge in, the bits of oxhip_rrt_batch_check_motion on the same two rows, for an edge of any length (a
 *     planted tree may hold such).  With unchanged obstacles every edge a kernel grew passes and the call changes nothing.
 *   Node 0 is never tested and always kept (setup() does not test the start); node i >= 1 stays iff edge_ok[i] and its parent
 *     stays.  Survivors keep their relative order: new_index[i] = survivors below i, -1 for a removed node; parents are remapped
 *     through new_index; n_nodes becomes the survivor count.  Tree, parents and skip flags afterwards are exactly what
 *     oxhip_rrt_batch_set_tree(problem, pruned states, pruned parents) leaves for a tree that set_tree planted or a kernel that
 *     keeps skip flags grew (a node carries the flag iff a SURVIVING node of lower index has equal coordinates).
 *   iterations, accepted, checksum and the RNG position do not change.
 *   goal_node becomes the lowest new index i >= 1 whose state satisfies the problem's goal (the planner's own comparison), -1 if
 *     there is none; the old value is not read (set_tree can leave it stale).  For a kernel-grown tree that is "the old goal node,
 *     remapped, if it survived".  goal_lost[p] = 1 iff goal_node was >= 0 and in range before and is -1 now.  stop_reason
 *     becomes OXHIP_STOP_NONE: the next solve runs the problem again.
 *   What set_tree drops is dropped for all problems: extracted / simplified paths, the binary32 shadows, the cell grids.  The
 *     next launch rebuilds them; this call rebuilds none.
 * n_removed[P], goal_lost[P]: may be NULL.  RRTConnect and RRT* batches: OXHIP_ERR_BAD_ARG (RRT* would need its costs and wiring
 * cursors pruned as well); SE(2) / SE(3) are RRTConnect only.  Without setup(): OXHIP_ERR_PLANNER_UNINITIALISED.  A refused call
 * changes nothing: extracted and simplified paths stay. */
int32_t oxhip_rrt_batch_revalidate_trees(oxhip_rrt_batch* b, uint32_t* n_removed /*[P] or NULL*/,
                                         uint8_t* goal_lost /*[P] or NULL*/);
/* new_index and edge_ok (edge_ok[0] = 1) of the last revalidate_trees for one problem, n_before entries each: a test hook, and
 * the way to remap per-node annotations of the caller's own.  Holds until the next setup / solve / set_tree / revalidate_trees;
 * after that, and before the first call, OXHIP_ERR_BAD_ARG.  cap < n_before: OXHIP_ERR_CAPACITY, *n_before still written. */
int32_t oxhip_rrt_batch_get_revalidate_map(oxhip_rrt_batch* b, uint32_t problem, int32_t* new_index /*[n_before] or NULL*/,
                                           uint8_t* edge_ok /*[n_before] or NULL*/, uint32_t cap, uint32_t* n_before);
/* HIP-event times (ms) of the last revalidate_trees: phase_ms[4] = {edge checks, survival, scan, compaction + remap + skip flags} */
int32_t oxhip_rrt_batch_revalidate_last_timing(oxhip_rrt_batch* b, double* phase_ms /*[4]*/);

/* Planner::solve (rrt.rs:158-227).  Runs every unfinished problem for at most max_iterations
 * further iterations (one iteration = one pass of rrt.rs:170-225).  timeout_s bounds wall time
 * (checked between kernel launches of at most 2048 iterations; 0 or +inf = none; NaN or negative =
 * OXHIP_ERR_BAD_ARG).  The planner mirrors above this ABI map the reference's `solve(Duration::ZERO)`
 * to PlanningError::Timeout themselves (rrt.rs:172-174 fails its first clock check).  Without a timeout
 * the budget is still cut into launches of 65,536 iterations so the host can see every problem stop.
 * freeze != 0 suppresses inserts
 * ("steady" measurement mode: every nearest-neighbour scan sees the same tree).
 * status_out[P] (may be NULL): OXHIP_OK if the problem has a goal node, else
 * OXHIP_ERR_NO_SOLUTION_FOUND / OXHIP_ERR_TIMEOUT.  Calling solve again continues the same
 * trees and RNG streams (the reference's tree also persists across solve calls). */
int32_t oxhip_rrt_batch_solve(oxhip_rrt_batch* b, uint64_t max_iterations, double timeout_s,
                              uint32_t freeze, int32_t* status_out);

/* per-problem counters (any pointer may be NULL) */
int32_t oxhip_rrt_batch_get_counts(oxhip_rrt_batch* b, uint64_t* iterations /*[P]*/,
                                   uint32_t* nodes /*[P]*/, uint64_t* accepted /*[P]*/,
                                   uint64_t* checksum /*[P]*/, int32_t* goal_node /*[P]*/,
                                   int32_t* stop_reason /*[P]*/);

/* RRT::tree of problem p (rrt.rs:61): states AoS [n][dim] and parent indices (-1 = None). */
int32_t oxhip_rrt_batch_get_tree(oxhip_rrt_batch* b, uint32_t problem, double* states,
                                 int32_t* parents, uint32_t cap_nodes, uint32_t* n_nodes);

/* reconstruct_path (rrt.rs:118-128) from the first goal node; len = 0 when unsolved. */
int32_t oxhip_rrt_batch_get_path(oxhip_rrt_batch* b, uint32_t problem, double* states,
                                 uint32_t cap_states, uint32_t* len);

/* RRTConnect only (rrt_connect.rs:58-59: start_tree / goal_tree).  get_tree / get_counts above address the
 * start tree (nodes[], goal_node[] = last start-tree node of the solution); these address the goal tree:
 * its size, the last goal-tree node of the solution (-1 when the start tree reached the goal itself,
 * rrt_connect.rs:271-274) and its nodes.  get_path returns the merged path of rrt_connect.rs:288-304. */
int32_t oxhip_rrt_batch_get_goal_counts(oxhip_rrt_batch* b, uint32_t* nodes /*[P]*/, int32_t* end_node /*[P]*/);
int32_t oxhip_rrt_batch_get_goal_tree(oxhip_rrt_batch* b, uint32_t problem, double* states, int32_t* parents,
                                      uint32_t cap_nodes, uint32_t* n_nodes);

/* RRT* only: Node::cost (rrt_star.rs:26) of every node of problem `problem`, in node order */
int32_t oxhip_rrt_batch_get_costs(oxhip_rrt_batch* b, uint32_t problem, double* costs, uint32_t cap_nodes,
                                  uint32_t* n_nodes);

/* ---- the whole batch's solution paths, extracted and shortcut on the device (path_simplify.hip extracts, shortcut_core.hip
 * shortcuts with every waypoint a row) ----
 * extract_paths walks the parent chain of every problem whose goal_node >= 0 on the device (RRTConnect: plus the goal-tree
 * chain, spliced as get_path splices it) and keeps the rows in path order behind a per-problem offset; an unsolved problem has
 * length 0.  Every space and planner a batch can hold.  get_paths hands everything out in one copy: problem p's path is rows
 * offsets[p] .. offsets[p+1] of `states`, and those rows equal oxhip_rrt_batch_get_path(p) bit for bit.  offsets / states may be
 * NULL; *total_out is always set, and cap_states < total is OXHIP_ERR_CAPACITY (the way get_path uses `len`).
 *
 * simplify_paths extracts the paths if that has not been done and shortcuts every one of them over its own waypoints.  The
 * semantics are this build's (the reference has no path simplifier).  Raw path p_0 .. p_{L-1}, span S = L - 1 when
 * max_span == 0, else min(max_span, L - 1); max_span == 1 leaves the path as it is.
 *   valid(i, j)   j == i + 1: true without a check (the planner accepted that edge; a goal-tree edge was checked in the other
 *                 direction).  2 <= j - i <= S: the batch's check_motion(from = p_i, to = p_j) -- the verdict of
 *                 oxhip_rrt_batch_check_motion on the same two rows.
 *   cost          cost[0] = 0; cost[j] = min over i in [j - S, j - 1] with valid(i, j) of fl(cost[i] + distance(p_i, p_j)), i
 *                 scanned ascending with strict '<' (ties keep the lowest i); distance is the space's own, in the bits of
 *                 oxhip_distance_batch / oxhip_so3_op_batch op 0.
 *   outputs       the simplified path is the parent chain from L - 1; simplified_cost = cost[L - 1]; raw_cost is the
 *                 left-to-right sum over adjacent edges.  Hence simplified_cost <= raw_cost exactly, and both ends are kept.
 * Built for OXHIP_SPACE_REAL_VECTOR (dim 2 .. 8, spheres and boxes, RRT / RRTConnect / RRT*), OXHIP_SPACE_SO3 and
 * OXHIP_SPACE_SO2 (an edge costs its SO(2) distance); SE(2) and SE(3) batches return OXHIP_ERR_BAD_ARG ("not built").  chunk_problems: problems per device round, 0 = automatic (a round's
 * bit matrices stay within 1 GiB; a single path whose matrix is larger is OXHIP_ERR_CAPACITY: pass a max_span); results never
 * depend on it.  get_simplified_paths: problem p's simplified states are rows offsets[p] .. offsets[p+1] of `states`, `indices`
 * their positions in the raw path; any of the three may be NULL.  get_simplify_results: per problem raw_cost, simplified_cost
 * and the number of motion checks evaluated (0 for an unsolved problem); any pointer may be NULL.
 *
 * The results belong to the trees as they stood at the call: a later setup, solve or set_tree discards them, and the getters
 * then return OXHIP_ERR_BAD_ARG ("no extracted / simplified paths"), as they do before the first call.  Without setup():
 * OXHIP_ERR_PLANNER_UNINITIALISED.  Neither call changes trees, counts or checksums. */
int32_t oxhip_rrt_batch_extract_paths(oxhip_rrt_batch* b);
int32_t oxhip_rrt_batch_get_paths(oxhip_rrt_batch* b, uint64_t* offsets /*[P+1]*/, double* states /*[total][dim]*/,
                                  uint64_t cap_states, uint64_t* total_out);
int32_t oxhip_rrt_batch_simplify_paths(oxhip_rrt_batch* b, uint32_t max_span, uint32_t chunk_problems);
int32_t oxhip_rrt_batch_get_simplified_paths(oxhip_rrt_batch* b, uint64_t* offsets /*[P+1]*/, double* states /*[total][dim]*/,
                                             uint32_t* indices /*[total]*/, uint64_t cap_states, uint64_t* total_out);
int32_t oxhip_rrt_batch_get_simplify_results(oxhip_rrt_batch* b, double* raw_cost /*[P]*/, double* simplified_cost /*[P]*/,
                                             uint64_t* checks /*[P]*/);
/* test hook: valid(i, j) of problem `problem`'s extracted path as the pair kernel evaluates it, out[i * L + j] for i < j within
 * the span (0 elsewhere), L * L bytes; *len_out = L; cap_bytes < L * L is OXHIP_ERR_CAPACITY */
int32_t oxhip_rrt_batch_path_valid_matrix(oxhip_rrt_batch* b, uint32_t problem, uint32_t max_span, uint8_t* out,
                                          uint64_t cap_bytes, uint32_t* len_out);
/* HIP-event times (ms) of the last extract_paths (both kernels) and of the last simplify_paths (pair matrix, DP), and its rounds */
int32_t oxhip_rrt_batch_paths_last_timing(oxhip_rrt_batch* b, double* extract_ms, double* pairs_ms, double* dp_ms,
                                          uint32_t* rounds);

/* HIP-event time (ms) of the kernels of the last solve call, their launch count, and which
 * kernel ran (oxhip_kernel_kind). */
int32_t oxhip_rrt_batch_last_timing(oxhip_rrt_batch* b, double* kernel_ms, uint32_t* launches,
                                    uint32_t* kernel_kind);

/* Diagnostics: in-kernel counters and cycle stamps of the resident kernels (a separately instantiated
 * diagnostic build; never time that build).  Up to OXHIP_STAMP_WORDS words; get_stamps writes
 * min(cap_words, OXHIP_STAMP_WORDS) of them.  rrt_lanes.hip (workgroup 0 unless noted): [1] resolver wait,
 * [2] work, [3] whole-tree-path cycles; [4] whole-tree-path events, [5] rounds, [6] lanes offered,
 * [7] iterations, [11] memoized answers used, [12] conflict cuts, [15] literal-loop ties,
 * [16+w] / [24+w] scanner wave w wait / work cycles, [32..39] resolver phases, [40..43] fold / conflict
 * trips and exact evaluations, [44..48] batch-wide maxima and sums, [50..53] audit (OXHIP_DEBUG_AUDIT),
 * [54] batch-wide whole-tree events, [55] memo hits, [56] conflict cuts, [57] ring wraps (rounds in which the
 * committed-node ring passed a multiple of its size), [58] two-lane passes.  rrt_cells.hip (problem 0, summed over the
 * parts of a split launch, unless noted): [4] whole-tree events, [5] rounds, [6] lanes offered, [7] iterations (an unsplit
 * launch adds the running total, a part its own count), [8] shell searches, [9] trips, [10] regrids, [11] memo hits,
 * [12] conflict cuts, [15] literal-loop ties; batch-wide: [14] ambiguous queries settled among the band nodes (counted in
 * [54] too), [50] / [51] / [52] sum, bitwise complement of the minimum, and maximum of the lifetimes of all waves, in cycles,
 * [53] lanes offered minus iterations run (0 in a frozen launch), [45] and [54] ambiguous-query events (band or whole tree), [55] memo hits, [56] conflict
 * cuts, [59] forced cuts (OXHIP_DEBUG_ONE_LANE_ROUNDS), [60] shell searches (past the first ring of cells), [61] regrids
 * inside a growing launch (not the prepare pass's builds), [3] (OXHIP_STAMP_CELLS_BOARD; written by get_stamps, not summed over
 * launches) the progress board of the last frozen launch as that launch left it, summed over the XCDs: every wave has reported
 * its whole quota, so it equals the live problems times oxhip_cells_problem_quota. */
#define OXHIP_STAMP_WORDS 64
#define OXHIP_STAMP_CELLS_BOARD 3
int32_t oxhip_rrt_batch_enable_stamps(oxhip_rrt_batch* b, uint32_t enable);
int32_t oxhip_rrt_batch_get_stamps(oxhip_rrt_batch* b, uint64_t* out, uint32_t cap_words);

/* rrt_cells.hip's frozen launches, host arithmetic only (no device is touched): how a launch of `rounds` rounds of 64 queries is
 * cut into `split` parts (1 .. 64), and the progress units the pacing of the parts counts in -- 16 per round a part runs, 1 per
 * round it skips over to reach its start (parts of a launch of up to 4 parts find their own starts).  part_begin: the first round
 * of part `part` (`rounds` for part >= split); part_quota: the units part `part` reports in all (0 for part >= split);
 * problem_quota: the parts' quotas together, which the launch hands to the kernel. */
uint32_t oxhip_cells_part_begin(uint32_t rounds, uint32_t part, uint32_t split);
uint64_t oxhip_cells_part_quota(uint32_t rounds, uint32_t part, uint32_t split);
uint64_t oxhip_cells_problem_quota(uint32_t rounds, uint32_t split);

/* ---- stand-alone batched primitives (same device functions as the planner kernels) ---- */

/* nearest-neighbour argmin of rrt.rs:187-196 for Q independent (tree, query) pairs:
 * nodes AoS [sum n_nodes][dim] concatenated, offsets via n_nodes[Q]; queries [Q][dim];
 * out: index (lowest index among post-sqrt ties) and min_dist = distance(nodes[idx], q). */
int32_t oxhip_nn_argmin_batch(int32_t device, uint32_t dim, const double* nodes,
                              const uint32_t* n_nodes, uint32_t n_queries, const double* queries,
                              uint32_t* out_index, double* out_min_dist);

/* RealVectorStateSpace::distance (rvss.rs:137-155) and ::interpolate (rvss.rs:161-186), n pairs */
int32_t oxhip_distance_batch(int32_t device, uint32_t dim, const double* a, const double* b,
                             uint32_t n, double* out);
int32_t oxhip_interpolate_batch(int32_t device, uint32_t dim, const double* from, const double* to,
                                const double* t, uint32_t n, double* out);

/* StateValidityChecker::is_valid for n states and RRT::check_motion (rrt.rs:90-116) for n
 * (from,to) pairs against the batch's current sphere/box field and space resolution (SE(2): segments; SO(3): cones,
 * interpolated as the SO(3) space does; SO(2): arcs, interpolated the shortest way round). */
int32_t oxhip_rrt_batch_is_valid(oxhip_rrt_batch* b, const double* states, uint32_t n, uint8_t* out);
int32_t oxhip_rrt_batch_check_motion(oxhip_rrt_batch* b, const double* from, const double* to,
                                     uint32_t n, uint8_t* out);

/* device arithmetic self-test hooks: out[i] = op(a[i], b[i]) computed on the GPU.
 * op: 0 sqrt(a), 1 a/b, 2 ceil(a), 3 a + (b - a) * t (t = c[i], unfused), 4 (a-b)*(a-b),
 *     5 / 6: sin(a) / cos(a) as the disc goal sampler evaluates them (ox_sincos; 0 <= a < 2^19 pi/2) */
int32_t oxhip_f64_op_batch(int32_t device, uint32_t op, const double* a, const double* b,
                           const double* c, uint32_t n, double* out);
/* SO(2) / SE(2) arithmetic self-test hooks, n rows of (x, y, theta):
 * op 0: out[i] = (se2_distance(a_i, b_i), so2_normalise(a_i.theta), so2_distance(a_i.theta, b_i.theta))
 * op 1: out[i] = se2_interpolate(a_i, b_i, t[i])        (so2_state_space.rs:97-122, so2_state.rs:33-37) */
int32_t oxhip_se2_op_batch(int32_t device, uint32_t op, const double* a, const double* b, const double* t, uint32_t n,
                           double* out);
/* SO(3) arithmetic self-test hooks (so3_state_space.rs:101-159), n rows of quaternions (x, y, z, w):
 * op 0: out[i] = distance(a_i, b_i)                       out[n]
 * op 1: out[i] = interpolate(a_i, b_i, t[i]), t in [0, 1]  out[n][4]
 * op 2: out[i] = ox_acos(a[i]), a read as n scalars (b and t may be NULL)   out[n] */
int32_t oxhip_so3_op_batch(int32_t device, uint32_t op, const double* a, const double* b, const double* t, uint32_t n,
                           double* out);
/* SE(3) arithmetic self-test hooks (OXHIP_SPACE_SE3), n rows of (x, y, z, qx, qy, qz, qw) in a and b:
 * op 0: out[i] = distance(a_i, b_i)                                              out[n]
 * op 1: out[i] = interpolate(a_i, b_i, t[i])                                     out[n][7]
 * op 2: out[i] = rot(q of a_i, first three of b_i) + xyz of a_i (t may be NULL)  out[n][3] */
int32_t oxhip_se3_op_batch(int32_t device, uint32_t op, const double* a, const double* b, const double* t, uint32_t n,
                           double* out);
/* device RNG self-test: the first n u64 words of the (seed, stream) ChaCha12 stream */
int32_t oxhip_rng_u64_batch(int32_t device, uint64_t seed, uint64_t stream, uint32_t n, uint64_t* out);

/* ---- PRM: replaces geometric::PRM (oxmpl/src/geometric/planners/prm.rs) ----
 *
 * PRM::new(timeout, connection_radius) (prm.rs:70-78) + RealVectorStateSpace::new.  The reference builds
 * its roadmap for `timeout` seconds of wall clock with an OS-seeded RNG; the device path adds the
 * deterministic caps max_milestones / max_samples (checked where the reference reads its clock,
 * prm.rs:118) and a ChaCha12 stream (seed, stream) restarted by setup().  For a given final milestone
 * count the roadmap does not depend on how construction was batched.
 *
 * space = OXHIP_SPACE_SO3: PRM over SO3StateSpace (prm_so3.hip).  dim must be 4 and the bounds are read as for an SO(3) RRT
 * batch: bounds[0..3] = centre quaternion, bounds[4] = max_angle (negative: OXHIP_ERR_ZERO_VOLUME; NaN reads as PI; clamped to
 * PI); lvs_fraction as there (res = 0.5 PI fraction 0.1).  States, start, goal centre and path rows are quaternions
 * (x, y, z, w).  oxhip_prm_set_spheres takes cones -- valid iff distance(centre, q) > radius for every cone (strict) --
 * and oxhip_prm_set_boxes and knn_k > 0 are OXHIP_ERR_BAD_ARG.  n_samples counts sample_uniform calls (accepted rejection
 * attempts).  Edges: distance < connection_radius (strict), check_motion with SO(3) interpolation; a radius above PI / 2 connects
 * every pair.  acos / sin are ox_acos / ox_sincos: PARITY UNPINNED against a libm-built oxmpl, as for SO(3) RRT. */
typedef struct oxhip_prm_config {
    uint32_t struct_size;               /* = sizeof(oxhip_prm_config) */
    uint32_t dim;                       /* 1..OXHIP_MAX_DIM */
    double   bounds[2 * OXHIP_MAX_DIM]; /* (lo,hi) pairs */
    double   timeout;                   /* PRM::timeout (prm.rs:50), seconds of construction; read between
                                           device rounds; <= 0 or inf: no wall-clock bound */
    double   connection_radius;         /* PRM::connection_radius (prm.rs:52): edge iff distance < radius (strict) */
    double   lvs_fraction;              /* longest_valid_segment_fraction, default 0.05 */
    uint32_t max_milestones;            /* construct_roadmap stops at this many milestones (build-defined) */
    int32_t  device;                    /* HIP device ordinal */
    uint64_t max_samples;               /* ... or after this many sample_uniform calls; 0 = 4096 * max_milestones + 2^22
                                           (so that a space with no valid state still returns) */
    uint64_t seed;                      /* ChaCha12 key = LE(seed)||0^24 */
    uint64_t stream;                    /* ChaCha12 stream id */
    uint32_t knn_k;                     /* 0: the reference's rule -- a new milestone connects to every earlier one within connection_radius
                                           (prm.rs:131-138).  k > 0: the k-nearest variant (BASELINE.json configs[4]: "all-pairs k-NN"): it connects
                                           to its k nearest earlier milestones, ordered by (distance, index), visited in ascending index order;
                                           check_motion and everything else as prm.rs.  The query's start connections keep the radius rule */
    uint32_t space;                     /* oxhip_space_kind: OXHIP_SPACE_REAL_VECTOR (0) or OXHIP_SPACE_SO3; anything else is
                                           OXHIP_ERR_BAD_ARG (this field was `reserved`, ignored, before) */
} oxhip_prm_config;

typedef struct oxhip_prm oxhip_prm;

int32_t oxhip_prm_create(const oxhip_prm_config* cfg, oxhip_prm** out);
int32_t oxhip_prm_destroy(oxhip_prm* prm);
/* the device-describable StateValidityChecker, as for the RRT batch */
int32_t oxhip_prm_set_spheres(oxhip_prm* prm, const double* centres /*[n][dim]*/, const double* radii, uint32_t n);
int32_t oxhip_prm_set_boxes(oxhip_prm* prm, const double* lo /*[n][dim]*/, const double* hi, uint32_t n);
/* Planner::setup (prm.rs:217-225): stores start / ball goal, clears the roadmap, restarts the RNG stream */
int32_t oxhip_prm_setup(oxhip_prm* prm, const double* start, const double* goal_centre, double goal_radius);
/* PRM::set_problem_definition (prm.rs:88-90): new start / goal, roadmap kept (multi-query use) */
int32_t oxhip_prm_set_problem(oxhip_prm* prm, const double* start, const double* goal_centre, double goal_radius);
/* PRM::construct_roadmap (prm.rs:96-154); a no-op when a roadmap exists (prm.rs:106-113) */
int32_t oxhip_prm_construct_roadmap(oxhip_prm* prm);
/* roadmap.len(), sum of edges.len() over all nodes (= 2 x undirected edges), sample_uniform calls made */
int32_t oxhip_prm_get_sizes(oxhip_prm* prm, uint32_t* n_milestones, uint64_t* n_edge_entries, uint64_t* n_samples);
/* PRM::get_roadmap (prm.rs:82-84): states AoS [n][dim]; node i's `edges` = neighbours[offsets[i] .. offsets[i+1]),
 * in the reference's order (ascending).  Any pointer may be NULL. */
int32_t oxhip_prm_get_roadmap(oxhip_prm* prm, double* states, uint32_t cap_nodes, uint64_t* offsets /*[n+1]*/,
                              uint32_t* neighbours, uint64_t cap_entries);
/* Planner::solve (prm.rs:227-307): OXHIP_OK and the path [start, milestones...] (prm.rs:189-208), or
 * OXHIP_ERR_PLANNER_UNINITIALISED / _UNSAMPLED_STATE_SPACE / _INVALID_START_STATE / _NO_SOLUTION_FOUND /
 * _TIMEOUT (graph search, prm.rs:285-287; timeout_s <= 0 or inf: none).  path may be NULL (length only). */
int32_t oxhip_prm_solve(oxhip_prm* prm, double timeout_s, double* path /*[cap_states][dim]*/, uint32_t cap_states,
                        uint32_t* len);
/* start_connections / goal_indices of the last solve (prm.rs:249-264) */
int32_t oxhip_prm_get_query_sets(oxhip_prm* prm, uint32_t* start_connections, uint32_t cap_start, uint32_t* n_start,
                                 uint32_t* goal_indices, uint32_t cap_goal, uint32_t* n_goal);
/* HIP-event times (ms) of the last construct_roadmap / solve: phase_ms[6] = {sampling, all-pairs radius
 * search, edge check_motion, key sort + CSR, query kernel, host BFS}; in-radius pairs examined; sample batches
 * replayed because rand's range sampler rejected a draw.  The phase times are the calls' own: oxhip_prm_grow_roadmap leaves
 * them as they were (its phases: oxhip_prm_grow_last_timing).  The pair count is the roadmap's: a grow adds the pairs it examined,
 * as it adds its exactly searched rows to oxhip_prm_knn_exact_rows. */
int32_t oxhip_prm_last_timing(oxhip_prm* prm, double* phase_ms /*[6]*/, uint64_t* n_candidates,
                              uint32_t* redraw_batches);
/* k-nearest variant, last construct_roadmap: rows whose candidate radius held fewer than k earlier milestones and that were
 * searched exactly instead (diagnostic: results do not depend on it) */
int32_t oxhip_prm_knn_exact_rows(oxhip_prm* prm, uint32_t* rows);

/* ---- a batch of queries on one roadmap, search included, on the device (prm_batch.hip) ----
 * n_queries (start, ball goal) pairs on the roadmap as it stands, each answered exactly -- bit for bit, status for status -- as
 * set_problem + solve answer it: start validity, start connections and goal milestones (prm.rs:243-264), the breadth-first
 * search (:270-301) and reconstruct_path (:189-208) all run on the device, one workgroup per query.  Per query:
 * OXHIP_ERR_INVALID_START_STATE, OXHIP_ERR_NO_SOLUTION_FOUND (no start connection, no goal milestone, or the search ran dry),
 * OXHIP_OK, or OXHIP_ERR_TIMEOUT.  chunk_queries: queries per device round, 0 = automatic (bounds the workspace: 9 bytes per
 * query and milestone, at most 1 GiB); results never depend on it.  timeout_s as the single solve reads it (<= 0, inf, NaN:
 * none); the clock is read between rounds: a query is either answered completely or OXHIP_ERR_TIMEOUT with length 0, and the
 * timed-out queries are a suffix of the batch (the first round always runs).  The call itself returns OXHIP_OK whatever the
 * queries' statuses, OXHIP_ERR_PLANNER_UNINITIALISED without setup(), OXHIP_ERR_UNSAMPLED_STATE_SPACE on an empty roadmap,
 * OXHIP_ERR_BAD_ARG for null pointers or a start / goal centre that set_problem would refuse; n_queries = 0 is OXHIP_OK.
 * The batch neither reads nor writes the handle's own problem definition or the last solve's query sets.  setup() (which
 * clears the roadmap) drops the batch's results -- the getters then return OXHIP_ERR_UNSAMPLED_STATE_SPACE, as they do before
 * the first batch; a new batch replaces them. */
int32_t oxhip_prm_solve_batch(oxhip_prm* prm, uint32_t n_queries, const double* starts /*[Q][dim]*/,
                              const double* goal_centres /*[Q][dim]*/, const double* goal_radii /*[Q]*/, double timeout_s,
                              uint32_t chunk_queries, int32_t* status_out /*[Q] or NULL*/);
/* per query of the last batch: status, path length in states (0 unless OXHIP_OK), the goal milestone reached (-1 unless
 * OXHIP_OK), |start_connections|, |goal_indices| (both 0 for an invalid start or a timed-out query, as after the single
 * solve).  Any pointer may be NULL. */
int32_t oxhip_prm_batch_get_results(oxhip_prm* prm, int32_t* status, uint32_t* path_len, int32_t* goal_node,
                                    uint32_t* n_start, uint32_t* n_goal);
/* all paths of the last batch in one copy: query q's path is rows offsets[q] .. offsets[q+1]; nodes = milestone index of
 * each row (0xFFFFFFFF for the start state, row 0 of every path); states = the rows themselves [total_rows][dim].
 * OXHIP_ERR_CAPACITY when cap_rows is too small; *total_rows and offsets are still written.  Any pointer may be NULL. */
int32_t oxhip_prm_batch_get_paths(oxhip_prm* prm, uint64_t* offsets /*[Q+1]*/, uint32_t* nodes, double* states,
                                  uint64_t cap_rows, uint64_t* total_rows);
/* start_connections / goal_indices of query `query` of the last batch, as the single-query getter returns them (the
 * flag kernel runs again for that query: the sets are not stored per query) */
int32_t oxhip_prm_batch_get_query_sets(oxhip_prm* prm, uint32_t query, uint32_t* start_connections, uint32_t cap_start,
                                       uint32_t* n_start, uint32_t* goal_indices, uint32_t cap_goal, uint32_t* n_goal);
/* HIP-event times (ms) of the last batch, summed over its rounds: phase_ms[4] = {flag kernel, search kernel, path
 * extraction, device-to-host copies}; the number of rounds */
int32_t oxhip_prm_batch_last_timing(oxhip_prm* prm, double* phase_ms /*[4]*/, uint32_t* rounds);

/* ---- the same batch answered with shortest paths (prm_shortest.hip) ----
 * The semantics are this build's own (the reference searches breadth-first only).  Per query, start validity, the start
 * connections S and the goal milestones G are exactly oxhip_prm_solve_batch's (the same flag kernels), and so are the statuses:
 * OXHIP_ERR_INVALID_START_STATE; OXHIP_ERR_NO_SOLUTION_FOUND when S or G is empty or no milestone of G has a finite label;
 * OXHIP_OK; OXHIP_ERR_TIMEOUT.  w(u, v) is the space's own distance between the milestones (the bits of oxhip_distance_batch /
 * oxhip_so3_op_batch op 0), init[m] = distance(start, m) for m in S and +inf elsewhere, and the labels c are the least solution of
 *     c[v] = min(init[v], min over neighbours u of fl(c[u] + w(u, v)))        (one rounded binary64 add per edge)
 * -- what Dijkstra computes.  An edge u -> v is tight iff fl(c[u] + w(u, v)) == c[v]; the sources are the m in S with
 * c[m] == init[m] (hops 0, parent = the start); hops[v] is v's breadth-first depth from the sources over tight edges and
 * parent[v] its lowest-index tight predecessor with hops[v] - 1.  The answer is the goal milestone of least (c, hops, index),
 * the path [start, chain ...] has hops + 2 states, and the left-to-right sum of its edge distances is c[goal] bit for bit.
 * weights: 0 = distance (above); 1 = every w and every init[m], m in S, is 1.0 (fewest hops under this tie rule); 2 = all of
 * them 0.0 (test only: every edge is tight); anything else is OXHIP_ERR_BAD_ARG.  Call-level statuses, argument checks,
 * chunk_queries (0 = automatic: 21 bytes per query and milestone, at most 1 GiB a round; results never depend on it) and the
 * timeout's suffix rule are oxhip_prm_solve_batch's.  The call becomes "the last batch": oxhip_prm_batch_get_results, _get_paths
 * and _get_query_sets serve it unchanged, and oxhip_prm_batch_last_timing reports phase_ms[4] = {flag kernel + initial labels,
 * label rounds + tight levels, path extraction, device-to-host copies} (the edge weights, computed once per roadmap -- 8 bytes
 * per CSR entry, kept until setup() -- are in none of them: see oxhip_prm_batch_get_search_stats).  It neither reads nor
 * writes the handle's own problem definition or the last single solve's query sets. */
int32_t oxhip_prm_solve_batch_shortest(oxhip_prm* prm, uint32_t n_queries, const double* starts /*[Q][dim]*/,
                                       const double* goal_centres /*[Q][dim]*/, const double* goal_radii /*[Q]*/, double timeout_s,
                                       uint32_t chunk_queries, uint32_t weights, int32_t* status_out /*[Q] or NULL*/);
/* c[goal] per query of the last batch, +inf where its status is not OXHIP_OK.  OXHIP_ERR_BAD_ARG when the last batch was an
 * oxhip_prm_solve_batch; OXHIP_ERR_UNSAMPLED_STATE_SPACE before any batch or after setup(), like the other getters. */
int32_t oxhip_prm_batch_get_costs(oxhip_prm* prm, double* cost /*[Q]*/);
/* test hook: all n labels of query `query` of the last shortest-path batch (flags, labels and levels run again for it, as
 * oxhip_prm_batch_get_query_sets re-runs the flags): cost = c (+inf: not reached), hops (0xFFFFFFFF where c is +inf), parent
 * (0x7FFFFFFF for a source, 0xFFFFFFFF where c is +inf).  Any pointer may be NULL; cap < n is OXHIP_ERR_CAPACITY. */
int32_t oxhip_prm_batch_get_labels(oxhip_prm* prm, uint32_t query, double* cost /*[n]*/, uint32_t* hops /*[n]*/,
                                   uint32_t* parent /*[n]*/, uint32_t cap);
/* diagnostics of the last shortest-path batch: per query the label rounds run and the edge relaxations evaluated; HIP-event
 * times (ms) summed over the rounds, phase_ms[6] = {edge weights (0 unless this batch computed them), flag kernel + initial
 * labels, label rounds, tight levels, path extraction, device-to-host copies}.  Any pointer may be NULL. */
int32_t oxhip_prm_batch_get_search_stats(oxhip_prm* prm, uint32_t* label_rounds /*[Q]*/, uint64_t* relaxations /*[Q]*/,
                                         double* phase_ms /*[6]*/);

/* ---- planting a roadmap from the host, re-checking a roadmap on the device (prm_revalidate.hip) ----
 * oxhip_prm_set_roadmap replaces the handle's roadmap with the caller's, in exactly the layout oxhip_prm_get_roadmap writes
 * (states AoS [n][dim]; node i's neighbours = neighbours[offsets[i] .. offsets[i+1])), for R^n (radius and k-nearest handles)
 * and SO(3).  OXHIP_ERR_BAD_ARG for a null argument (neighbours may be NULL when offsets[n] == 0),
 * OXHIP_ERR_PLANNER_UNINITIALISED without setup(), OXHIP_ERR_CAPACITY when n > max_milestones or offsets[n] > 0xFFFFFFFF.
 * n == 0 is OXHIP_OK and leaves an empty roadmap (construct_roadmap builds again).  Every coordinate must be finite and within
 * 1e150 (what set_problem asks of a start); a state need not lie inside the bounds and is not normalised.  The structure is
 * checked on the device: offsets[0] == 0 and offsets non-decreasing; every neighbour < n; no self-loop; every row strictly
 * ascending; symmetric (v in row u implies u in row v).  A violation is OXHIP_ERR_BAD_ARG, and oxhip_last_error_string() names
 * the first violated rule in that order (offsets_start, offsets_order, neighbour_range, self_loop, unsorted, asymmetric) and the
 * lowest offending row.  A refused call leaves the handle exactly as it was.  Success sets n_samples = 0 and drops what
 * belonged to the old roadmap, as setup() does: the last solve's query sets, the last batch's results, the edge weights.
 * construct_roadmap afterwards is the no-op it is for any existing roadmap; setup() clears a planted roadmap like any other. */
int32_t oxhip_prm_set_roadmap(oxhip_prm* prm, const double* states /*[n][dim]*/, uint32_t n, const uint64_t* offsets /*[n+1]*/,
                              const uint32_t* neighbours);
/* Re-checks the roadmap as it stands against the handle's CURRENT spheres / boxes / cones (the semantics are this build's own;
 * the reference has no such call).  valid[i] = is_valid(milestone i), the bits of oxhip_rrt_batch_is_valid on an RRT batch of
 * the same space, bounds, fraction and obstacles.  An undirected edge {i < j} is kept iff valid[i], valid[j] and
 * check_motion(from = milestone j, to = milestone i) -- construction's own direction (prm.rs:134).  Milestone indices are
 * stable: an invalid milestone stays in place as a row with no entries (check_motion tests its `to` state, so it can never
 * become a start connection, and no search reaches it).  Rows stay ascending.  milestone_valid [n] receives valid,
 * *n_invalid_milestones its zeros, *n_removed_entries = entries before - entries after; any of the three may be NULL.  Drops
 * the same derived state as oxhip_prm_set_roadmap (the batch getters answer as after setup()).
 * OXHIP_ERR_PLANNER_UNINITIALISED without setup(), OXHIP_ERR_UNSAMPLED_STATE_SPACE on an empty roadmap. */
int32_t oxhip_prm_revalidate(oxhip_prm* prm, uint8_t* milestone_valid /*[n] or NULL*/, uint32_t* n_invalid_milestones,
                             uint64_t* n_removed_entries);
/* HIP-event times (ms) of the last oxhip_prm_revalidate: phase_ms[4] = {milestone validity, pair emission, edge checks,
 * compaction (scan + move)} */
int32_t oxhip_prm_revalidate_last_timing(oxhip_prm* prm, double* phase_ms /*[4]*/);

/* ---- growing a roadmap in place (prm_grow.hip) ----
 * oxhip_prm_grow_roadmap continues the reference's construction loop (prm.rs:117-147) on the roadmap as it stands -- built,
 * planted or re-checked -- under the obstacles as they are now: OMPL's PRM::growRoadmap.  The semantics are this build's own.
 * Bounded by counts, not by cfg.timeout.  Old milestone indices, states and the old part of every old row do not change; new
 * milestones get the indices n, n + 1, ... in sample order.  An old milestone i is LIVE iff is_valid(milestone i) holds now
 * (oxhip_prm_revalidate's milestone test, evaluated when the call starts); a new milestone is live.  A new milestone j gets the
 * edge {i < j} iff i is live, distance(j, i) < connection_radius (strict, construction's device test) and
 * check_motion(from = j, to = i) -- the rule oxhip_prm_revalidate keeps edges by, so a re-check right after a grow removes
 * nothing.  A dead milestone keeps its row and gets no new entry.  k-nearest handles (knn_k > 0): a new row takes its k nearest
 * earlier milestones as construction does; with any dead milestone the call is OXHIP_ERR_BAD_ARG (k-nearest growth over invalid
 * milestones is not built).
 * Sampler: flags = 0 continues the handle's stream at the word where its last construct_roadmap / grow_roadmap stopped, so
 * construct to N1 + grow N2 equals construct to N1 + N2 bit for bit (with cfg.timeout = 0).  revalidate, set_spheres, set_boxes
 * and set_problem keep that position; setup and set_roadmap forget it, and a handle without one refuses flags = 0 with
 * OXHIP_ERR_BAD_ARG (starting silently at word 0 would re-draw the milestones a saved roadmap was built from).
 * OXHIP_PRM_GROW_NEW_STREAM starts at word 0 of stream `stream` (key = cfg.seed), which becomes the handle's stream for later
 * default grows.  n_samples (oxhip_prm_get_sizes) keeps counting from where it stood, 0 after set_roadmap.
 * Capacity: n + n_more may exceed cfg.max_milestones, up to 2^26 in all (beyond: OXHIP_ERR_CAPACITY); the handle's buffers are
 * then moved once to the next power of two.
 * OXHIP_ERR_BAD_ARG for a null pointer, a wrong struct_size, n_more = 0 or an unknown flag (before any device call);
 * OXHIP_ERR_PLANNER_UNINITIALISED without setup(); OXHIP_ERR_UNSAMPLED_STATE_SPACE on an empty roadmap (construct_roadmap
 * builds one).  max_samples exhausted is OXHIP_OK with *n_added < n_more.  A refused call leaves the handle as it was.
 * Success drops what belonged to the roadmap before, as oxhip_prm_revalidate does. */
#define OXHIP_PRM_GROW_NEW_STREAM 1u
typedef struct {
    uint32_t struct_size;
    uint32_t n_more;        /* milestones to add; 0 is OXHIP_ERR_BAD_ARG */
    uint64_t max_samples;   /* sample_uniform calls this call may make; 0 = 4096 * n_more + 2^22, construct's rule */
    uint32_t flags;         /* OXHIP_PRM_GROW_NEW_STREAM = 1 */
    uint32_t pad;
    uint64_t stream;        /* with NEW_STREAM: the ChaCha12 stream id to start at word 0 of (key = cfg.seed) */
} oxhip_prm_grow_config;
int32_t oxhip_prm_grow_roadmap(oxhip_prm* prm, const oxhip_prm_grow_config* g, uint32_t* n_added, uint64_t* n_samples_drawn);
/* HIP-event times (ms) of the last oxhip_prm_grow_roadmap: phase_ms[6] = {liveness mask, keys from CSR, sample,
 * pairs (+ filter), edges, sort + CSR} */
int32_t oxhip_prm_grow_last_timing(oxhip_prm* prm, double* phase_ms /*[6]*/);

/* ---- the roadmap as a graph: connected components, and pruning (prm_components.hip) ----
 * label[i] = the lowest milestone index of i's connected component (so label[i] <= i and label[label[i]] == label[i]);
 * size[i] = the number of milestones in i's component.  A row without entries -- isolated or dead -- is a component of its own.
 * Only the CSR is read: no obstacle, no state.  *largest_label = the label of the component with the most milestones, ties to the
 * lowest label; *largest_size its size.  Any out pointer may be NULL; label/size non-NULL with cap < n: OXHIP_ERR_CAPACITY.
 * OXHIP_ERR_BAD_ARG for a null handle, OXHIP_ERR_PLANNER_UNINITIALISED without setup(), OXHIP_ERR_UNSAMPLED_STATE_SPACE on an
 * empty roadmap.  The labels stay on the device until the roadmap changes, so a second call only copies. */
int32_t oxhip_prm_components(oxhip_prm* prm, uint32_t* label /*[n]*/, uint32_t* size /*[n]*/, uint32_t cap,
                             uint32_t* n_components, uint32_t* largest_label, uint32_t* largest_size);
/* HIP-event times (ms) of the last oxhip_prm_components: phase_ms[4] = {init + hook, flatten, sizes + summary, copies} (the first
 * three are 0 when the call was answered from the labels kept on the device); *launches = the kernels a computation launches,
 * a constant of the code that does not depend on the graph.  Either pointer may be NULL. */
int32_t oxhip_prm_components_last_timing(oxhip_prm* prm, double* phase_ms /*[4]*/, uint32_t* launches);

/* oxhip_prm_prune removes milestones and renumbers the rest.  The semantics are this build's own: the reference has no such call.
 * Two stages.  Stage 1: a milestone survives iff every requested one of INVALID (is_valid holds now) and MASK (keep[i] != 0)
 * holds.  Stage 2: MIN_SIZE and LARGEST are evaluated on the components of the graph that survives stage 1 -- an entry with a
 * dropped end connects nothing -- so INVALID | LARGEST drops, in the same call, the smaller piece an invalid cut milestone
 * leaves behind.  Survivors keep their relative order (new_index is monotone), so rows stay ascending and symmetric; an entry
 * stays iff both its ends stay; states move bit for bit (with the binary32 shadow of an R^n handle).  Not a re-check: an edge
 * between two kept milestones is never tested.  n_samples, the sampler's stream position (a default grow still works) and the
 * capacity stay as they are.  Derived state is dropped as oxhip_prm_revalidate drops it, whether or not anything was removed:
 * the host copy, the last solve's query sets, the last batch's results, the edge weights, the kept component labels.
 * new_index [n before the call] (or NULL) receives where each milestone went, -1 = dropped; *n_kept and *n_removed_entries
 * may be NULL.  R^n radius, R^n k-nearest and SO(3) handles alike.
 * Refused before the handle is read, OXHIP_ERR_BAD_ARG: a null handle or config, a wrong struct_size, flags == 0 or an unknown
 * flag, pad != 0, MASK without keep or keep without MASK, MIN_SIZE with min_size == 0.  Then OXHIP_ERR_PLANNER_UNINITIALISED
 * without setup(), OXHIP_ERR_UNSAMPLED_STATE_SPACE on an empty roadmap, and OXHIP_ERR_BAD_ARG ("would keep no milestone") when
 * nothing would survive.  A refused call leaves the handle exactly as it was. */
#define OXHIP_PRM_PRUNE_INVALID  1u   /* drop milestones whose is_valid is false NOW (revalidate's milestone test) */
#define OXHIP_PRM_PRUNE_MASK     2u   /* drop milestones with keep[i] == 0 */
#define OXHIP_PRM_PRUNE_MIN_SIZE 4u   /* drop components with fewer than min_size milestones */
#define OXHIP_PRM_PRUNE_LARGEST  8u   /* keep only the largest component (ties: lowest label) */
typedef struct {
    uint32_t struct_size;
    uint32_t flags;         /* OXHIP_PRM_PRUNE_*, at least one */
    uint32_t min_size;      /* with MIN_SIZE: at least 1 */
    uint32_t pad;           /* 0 */
} oxhip_prm_prune_config;   /* 16 bytes */
int32_t oxhip_prm_prune(oxhip_prm* prm, const oxhip_prm_prune_config* c, const uint8_t* keep /*[n] iff MASK*/,
                        int32_t* new_index /*[n_before] or NULL: -1 = dropped*/, uint32_t* n_kept, uint64_t* n_removed_entries);
/* HIP-event times (ms) of the last oxhip_prm_prune: phase_ms[5] = {masks, components, scans, move entries, move states} */
int32_t oxhip_prm_prune_last_timing(oxhip_prm* prm, double* phase_ms /*[5]*/);

/* ---- the handle's own checker, and the last batch's paths subdivided and shortcut (prm_path_simplify.hip subdivides and compacts,
 * shortcut_core.hip shortcuts) ----
 * is_valid / check_motion: the handle's StateValidityChecker and the check_motion that construction uses, over caller rows
 * ([n][dim]; SO(3): quaternions), against the obstacles as they are at the call; for every handle kind (radius, k-nearest,
 * SO(3)), with or without a roadmap.  Without setup(): OXHIP_ERR_PLANNER_UNINITIALISED. */
int32_t oxhip_prm_is_valid(oxhip_prm* prm, const double* states /*[n][dim]*/, uint32_t n, uint8_t* out /*[n]*/);
int32_t oxhip_prm_check_motion(oxhip_prm* prm, const double* from /*[n][dim]*/, const double* to /*[n][dim]*/, uint32_t n,
                               uint8_t* out /*[n]*/);
/* oxhip_prm_batch_simplify_paths shortcuts every OXHIP_OK path of the last batch (oxhip_prm_solve_batch or _shortest) on the
 * device.  The semantics are this build's own, as section 18's are:
 *   The dense path.  Query q has the raw path p_0 .. p_{L-1} of oxhip_prm_batch_get_paths and m = subdivide >= 1.  The dense path
 *     has M = (L - 1) m + 1 points: q_{k m} = p_k, copied as 64-bit words (a -0.0 or an unnormalised quaternion keeps its bits),
 *     and q_{k m + r} = interpolate(p_k, p_{k+1}, t) for 0 < r < m with t = (double)r / (double)m, one correctly rounded divide;
 *     the interpolation is the space's own, unfused: the bits of oxhip_interpolate_batch for R^n and of the interpolate op of
 *     oxhip_so3_op_batch for SO(3).
 *   Window.  S = L - 1 when max_span == 0, else min(max_span, L - 1), counted in original edges; W = S m in dense indices.
 *     max_span == 1 with m == 1 leaves the path as it is.
 *   valid(u, v) for u < v <= u + W.  True without a check when both points lie on one original edge, floor(u / m) ==
 *     floor((v - 1) / m): the roadmap accepted that motion and this is a part of it (for m == 1: "adjacent is valid").
 *     Otherwise the handle's check_motion, from = q_u, to = q_v, in path order, against the obstacles as they are at the call:
 *     the verdict of oxhip_prm_check_motion on the same two rows.
 *   Cost.  cost[0] = 0; cost[v] = the minimum of fl(cost[u] + distance(q_u, q_v)) over u in [v - W, v - 1] with valid(u, v),
 *     u scanned ascending with strict '<' (ties keep the lowest u); the distance is the space's own (the bits of
 *     oxhip_distance_batch / oxhip_so3_op_batch op 0).
 *   Outputs.  The simplified path is the parent chain from M - 1, with its dense indices; both ends are kept.
 *     simplified_cost = cost[M - 1]; raw_cost = the left-to-right sum over the original edges p_k -> p_{k+1} (after a
 *     weights = 0 shortest batch: oxhip_prm_batch_get_costs's c[goal] bit for bit); simplified_cost <= raw_cost holds exactly,
 *     since every hop q_{k m} -> q_{(k+1) m} is in the window and rounding is monotone.  checks = the number of pairs of the
 *     window that are not on one edge.  A query whose status is not OXHIP_OK has length 0, both costs 0.0 and checks 0.
 * Spaces: R^1 .. R^8 (spheres and boxes; radius and k-nearest handles) and SO(3).  subdivide 0 or above 256 is
 * OXHIP_ERR_BAD_ARG.  chunk_queries: queries per device round, 0 = automatic (a round's bit matrices -- bit (d - 2) M + u for
 * d = v - u in [2, W], whole 64-bit words per query -- stay within 1 GiB; one path whose matrix is larger is
 * OXHIP_ERR_CAPACITY: pass a max_span or a smaller subdivide); results never depend on it.
 * Without setup(): OXHIP_ERR_PLANNER_UNINITIALISED.  Without a current batch (none yet, or after setup()) simplify and its
 * getters answer OXHIP_ERR_UNSAMPLED_STATE_SPACE, as the batch getters do; with a batch but no simplify since it the getters
 * return OXHIP_ERR_BAD_ARG ("no simplified paths").  A new batch, setup() and every call that changes the roadmap (set_roadmap,
 * revalidate, grow_roadmap, prune, construct_roadmap) drop the results; set_spheres / set_boxes do not: the next simplify
 * reads the new obstacles.  Simplify changes neither the roadmap, the batch's own results nor the single-query state; a refused
 * simplify (OXHIP_ERR_BAD_ARG, OXHIP_ERR_CAPACITY) leaves the last results as they were.
 * get_simplified_paths: query q's simplified states are rows offsets[q] .. offsets[q+1] of `states`, `indices` their dense
 * indices u; any of the three may be NULL.  get_simplify_results: any pointer may be NULL. */
int32_t oxhip_prm_batch_simplify_paths(oxhip_prm* prm, uint32_t subdivide, uint32_t max_span, uint32_t chunk_queries);
int32_t oxhip_prm_batch_get_simplified_paths(oxhip_prm* prm, uint64_t* offsets /*[Q+1]*/, double* states /*[total][dim]*/,
                                             uint32_t* indices /*[total]*/, uint64_t cap_rows, uint64_t* total_rows);
int32_t oxhip_prm_batch_get_simplify_results(oxhip_prm* prm, double* raw_cost /*[Q]*/, double* simplified_cost /*[Q]*/,
                                             uint64_t* checks /*[Q]*/);
/* test hook: valid(u, v) of query `query`'s dense path as the pair kernel evaluates it, out[u * M + v] for u < v within the
 * window (same-edge pairs read 1; 0 elsewhere), M * M bytes; *len_out = M (0: no path); out == NULL only asks for M;
 * cap_bytes < M * M is OXHIP_ERR_CAPACITY.  It leaves the last simplify's results as they are. */
int32_t oxhip_prm_batch_path_valid_matrix(oxhip_prm* prm, uint32_t query, uint32_t subdivide, uint32_t max_span, uint8_t* out,
                                          uint64_t cap_bytes, uint32_t* len_out);
/* HIP-event times (ms) of the last oxhip_prm_batch_simplify_paths, summed over its rounds: phase_ms[4] = {upload + subdivide,
 * pair matrix, DP, gather + device-to-host copies}; the number of rounds.  Either pointer may be NULL; without setup():
 * OXHIP_ERR_PLANNER_UNINITIALISED, as the other calls of this section. */
int32_t oxhip_prm_batch_simplify_last_timing(oxhip_prm* prm, double* phase_ms /*[4]*/, uint32_t* rounds);

#ifdef __cplusplus
}
#endif
#endif /* OXMPL_HIP_H */
