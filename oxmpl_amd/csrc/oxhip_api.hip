// oxhip_api.hip -- implementation of the C ABI declared in include/oxmpl_hip.h.
//
// Host side of the drop-in boundary: validates what the reference would reject or panic on
// (real_vector_state_space.rs:69-93,239-244; rand's Bernoulli::new), precomputes the values
// the reference recomputes per call (extent, lvsl: rvss.rs:103-118,251-253), owns the device
// buffers and launches the kernels.  There is no CPU fallback: without a HIP device every
// entry point that computes returns OXHIP_ERR_NO_DEVICE.
#include "../../include/oxmpl_hip.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "oxhip_host.hpp"
#include "oxhip_internal.hpp"
#include "rrt_device.hpp"

using namespace oxhip;

#include <mutex>
#include <utility>
namespace {
std::mutex g_stream_mu;
std::vector<std::pair<int, hipStream_t>> g_stream_pool;
constexpr size_t kStreamPoolMax = 32;
}
namespace oxhip {
hipError_t oxhip_stream_acquire(int device, hipStream_t* out) {
    {
        std::lock_guard<std::mutex> lk(g_stream_mu);
        for (size_t i = g_stream_pool.size(); i-- > 0;)
            if (g_stream_pool[i].first == device) {
                *out = g_stream_pool[i].second;
                g_stream_pool.erase(g_stream_pool.begin() + (long)i);
                return hipSuccess;
            }
    }
    return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}
void oxhip_stream_release(int device, hipStream_t s) {
    if (!s) return;
    (void)hipStreamSynchronize(s);
    {
        std::lock_guard<std::mutex> lk(g_stream_mu);
        if (g_stream_pool.size() < kStreamPoolMax) { g_stream_pool.emplace_back(device, s); return; }
    }
    (void)hipStreamDestroy(s);
}
}  // namespace oxhip

// ------------------------------------------------------------------ the handle, in parts
// Each part owns its buffers, its flags and -- where it is a service with phase times -- those times and its clock.  bind() is the
// one place that copies a part's device pointers (and counts) into DevParams; it is called where the part's buffers are allocated
// or replaced.  (Cells carves one arena: alloc_cells computes its pointers and stores them at the same place.)
struct Trees {                        // what the planners grow
    DevBuf<double> tree, tree_b;      // [P][dim][cap]; tree_b: RRTConnect's goal trees
    DevBuf<int32_t> parent, parent_b;
    DevBuf<uint8_t> skip;
    DevBuf<ProblemState> state;
    ProblemState* h_states = nullptr;   // pinned: the state array as the host reads it after every launch
    ~Trees() { if (h_states) (void)hipHostFree(h_states); }
    void bind(DevParams& dp) const {
        dp.tree = tree.p; dp.parent = parent.p; dp.skip = skip.p; dp.state = state.p;
        dp.tree_b = tree_b.p; dp.parent_b = parent_b.p;
    }
};
struct Goals {
    DevBuf<double> goal_c, goal_thr, goal_r;
    std::vector<double> starts;       // host copy, [P][dim]
    void bind(DevParams& dp) const { dp.goal_c = goal_c.p; dp.goal_thr = goal_thr.p; dp.goal_r = goal_r.p; }
};
struct Obstacles {
    uint32_t n_spheres = 0, n_boxes = 0, n_segs = 0;
    DevBuf<double> sph_c, sph_thr, box_lo, box_hi;
    std::vector<double> sph_centres, sph_radii;   // host copies (AoS) for the filter thresholds
    DevBuf<double> sph_r;             // the radii as given: uploaded by upload_radii alone, when set_spheres changed them
    bool radii_dirty = true;
    DevBuf<double> segs;              // SE(2): segment soup
    DevBuf<uint16_t> seg_grid;        // ... and the cells' segment lists (rrt_connect_se2.hip, seg_grid_kernel)
    DevBuf<double> se3_body;          // SE(3): the body's spheres, SoA [4][kSe3MaxBody] (rrt_connect_se3.hip)
    Se3Args se3{};
    // the filters refresh_filter derives from spheres, starts and bounds before a launch reads them
    bool filt_dirty = true;
    DevBuf<double> sph_filt;          // the midpoint filter's thresholds
    DevBuf<uint64_t> conn_grid;       // RRTConnect in R^2 / R^3: the spheres that reach each cell of the bounds' grid (rrt_connect.hip)
    DevBuf<double> conn_filt;
    // (the grids in use -- dp.seg_grid, dp.sph_grid, dp.star_sph_grid -- are decisions of the calls that build them, not bindings)
    void bind(DevParams& dp) {
        dp.n_spheres = n_spheres; dp.sph_c = sph_c.p; dp.sph_thr = sph_thr.p; dp.sph_r = sph_r.p; dp.sph_filt = sph_filt.p;
        dp.n_boxes = n_boxes; dp.box_lo = box_lo.p; dp.box_hi = box_hi.p;
        dp.n_segs = n_segs; dp.segs = segs.p;
        se3.body = se3_body.p;
    }
};
// rrt_cells.hip: cell blocks, flat lists of small trees, node-major coordinates, grid descriptors, accumulators and part
// positions of split frozen launches, the sphere mask grid -- ONE allocation (a hipMalloc costs more than a small kernel:
// the one-problem Planner::solve pays for every one of them), carved at 256-byte boundaries
struct Cells {
    DevBuf<uint8_t> arena;
    CellMeta* meta = nullptr;
    uint64_t* sph_grid = nullptr;
    uint64_t* star_grid = nullptr;    // RRT*'s edge checks: the mask grid for motions up to search_radius long
    int32_t board_last = -1;          // parity of the last frozen cells launch (its progress board: get_stamps), -1: none yet
};
struct Shadow {                       // stream / RRT* kernels: fl32 shadow of the tree
    DevBuf<float> tree32;
    DevBuf<uint32_t> state;           // [P][2]
    void bind(DevParams& dp) const { dp.tree32 = tree32.p; dp.shadow_state = state.p; }
};
struct Solve {
    uint32_t kernel_kind = OXHIP_KERNEL_STREAM;   // the kind create() resolved (KERNEL_AUTO among them): every launch uses it, last_timing reports it
    double last_kernel_ms = 0.0;
    uint32_t last_launches = 0;
    enum { kBegin, kEnd };
    PhaseClock clk{2};                // made with the handle: create() has the device current
};
// path_simplify.hip, shortcut_core.hip: the batch's solution paths as extract_paths / simplify_paths left them.  They belong to the trees as they
// stood at that call (drop_derived, below).
struct Paths {
    bool ok = false, simp_ok = false;
    std::vector<uint64_t> off;                    // [P + 1] host copy of the row offsets
    std::vector<uint32_t> h_len;                  // [P]
    DevBuf<uint64_t> d_off, sp_woff, sp_bits, sp_checks;
    DevBuf<uint32_t> len, len_a, sp_par, sp_idx, sp_len;
    DevBuf<double> rows, sp_cost, sp_raw, sp_simp;
    double ms[3] = {0.0, 0.0, 0.0};               // extraction kernels, pair matrix, DP of the last calls
    uint32_t rounds = 0;
    enum { kBegin, kMid, kEnd };                  // extract_paths: kBegin .. kMid per kernel; simplify_paths: pairs, then the DP
    std::unique_ptr<PhaseClock> clk;              // made by the first call that times itself and kept, as the workspace is
    void drop() { ok = simp_ok = false; }         // extract_paths: the paths start over; the trees, and a map of theirs, stay
};
// rrt_revalidate.hip: the workspace of revalidate_trees (allocated on first use and kept) and the map of its last call, which
// belongs to the trees as that call left them (drop_derived, below)
struct Reval {
    bool ok = false;
    DevBuf<uint8_t> edge_ok, alive, goal_lost, stage;
    DevBuf<int32_t> new_index, jump;
    DevBuf<uint32_t> n_after, n_removed;
    std::vector<uint32_t> n_before;               // [P] tree sizes before the last call
    double ms[4] = {0.0, 0.0, 0.0, 0.0};          // edge checks, survival, scan, compaction + remap + skip flags
    enum { kBegin, kEdgesEnd, kSurviveEnd, kScanEnd, kCompactEnd };   // ms[i]: mark i to mark i + 1
    std::unique_ptr<PhaseClock> clk;              // as Paths::clk
};
struct Star {                         // RRT*
    DevBuf<double> cost;              // cost-to-come
    DevBuf<uint64_t> wire_chk;        // W of the checksum
    DevBuf<uint32_t> nb_idx;          // the one-kernel design's neighbour scratch (rrt_star.hip)
    DevBuf<double> nb_dist;
    // the decoupled design (rrt_star_wire.hip): geometry by rrt_lanes.hip / rrt_cells.hip, then the wiring kernels
    struct Wiring {
        bool on = false;              // this design runs (else rrt_star.hip)
        bool geo_cells = false;       // ... its geometry by rrt_cells.hip
        DevBuf<StarEntry> pool;
        DevBuf<StarChunk> chunks;
        DevBuf<uint32_t> chunk_cursor, wired, nbr_cnt, nbr_off, nbr_take, nbr_total;
        DevBuf<double> d_near, star_filt;
        PooledStream stream2;         // the wiring of a segment runs here while the next segment's pairs are checked on the handle's stream
        hipEvent_t ev_seg[8] = {}, ev_join = nullptr;
        void release() {              // the buffers create() allocates for it (KERNEL_AUTO's fallback to the one-kernel design)
            pool.release(); chunks.release(); chunk_cursor.release(); wired.release(); nbr_take.release();
            nbr_total.release(); nbr_cnt.release(); nbr_off.release(); d_near.release();
        }
        ~Wiring() {
            stream2.close();
            for (hipEvent_t ev : ev_seg) if (ev) (void)hipEventDestroy(ev);
            if (ev_join) (void)hipEventDestroy(ev_join);
        }
    } wiring;
    void bind(DevParams& dp) const {
        dp.cost = cost.p; dp.wire_chk = wire_chk.p; dp.nb_idx = nb_idx.p; dp.nb_dist = nb_dist.p;
        dp.wired = wiring.wired.p; dp.nbr_cnt = wiring.nbr_cnt.p; dp.nbr_off = wiring.nbr_off.p; dp.nbr_take = wiring.nbr_take.p;
        dp.nbr_total = wiring.nbr_total.p; dp.d_near = wiring.d_near.p; dp.pool = wiring.pool.p;
        dp.chunks = wiring.chunks.p; dp.chunk_cursor = wiring.chunk_cursor.p;
    }
};

// destroy() makes the device current and drains the stream; the members then go in reverse order of declaration, which is the
// order the resources need: the second stream released, the events destroyed, the stream released, the pinned memory freed, each
// part's buffers with it.
struct oxhip_rrt_batch {
    oxhip_rrt_config cfg{};
    DevParams dp{};
    bool is_setup = false;
    DevBuf<uint64_t> dbg;             // enable_stamps
    Goals goals;
    Obstacles obs;
    Cells cells;
    Shadow shadow;
    Trees trees;
    PooledStream stream;
    Solve solve;
    Paths paths;
    Reval reval;
    Star star;
};

// What belongs to the trees as they stood is dropped when they change.  Two rules, and every entry point that changes trees or
// paths calls exactly one of them:
//   drop_derived  -- setup, solve, set_tree and an accepted revalidate_trees: the extracted paths, the simplified paths and the
//                    re-check map all go (their getters refuse until the service runs again);
//   Paths::drop   -- extract_paths: the paths start over (simplified ones with them), the trees stay and so does their map.
// (simplify_paths clears simp_ok alone: it keeps the paths it shortcuts.)  tests/test_gpu_rrt_handle_contract.py asserts this.
static void drop_derived(oxhip_rrt_batch* b) { b->paths.drop(); b->reval.ok = false; }

// The derived device state of `count` problems' trees from `first` on starts over: the fl32 shadows and the cell grids, which
// the kernels rebuild from the trees.  The only place that does; setup, set_tree and revalidate_trees call it, on the stream.
static int32_t reset_tree_caches(oxhip_rrt_batch* b, uint32_t first, uint32_t count) {
    if (b->shadow.state.p) HIP_TRY(hipMemsetAsync(b->shadow.state.p + 2 * (size_t)first, 0, (size_t)count * 2 * sizeof(uint32_t), b->stream));
    if (b->cells.meta) HIP_TRY(hipMemsetAsync(b->cells.meta + first, 0, (size_t)count * sizeof(CellMeta), b->stream));
    b->dp.cells_meta_ok = 0;
    return OXHIP_OK;
}

// sph_r's one owner: the radii travel when set_spheres changed them since the last upload, and not otherwise.
static int32_t upload_radii(oxhip_rrt_batch* b) {
    if (b->obs.radii_dirty) {
        OX_TRY(upload(b->obs.sph_r, b->obs.sph_radii, b->stream));
        b->obs.radii_dirty = false;
        b->obs.bind(b->dp);
    }
    return OXHIP_OK;
}

// a service's clock: made by its first call (the device is current) and kept
static int32_t clock_of(std::unique_ptr<PhaseClock>& clk, int n) {
    if (!clk) clk.reset(new PhaseClock(n));
    if (clk->made != hipSuccess) {
        const hipError_t e = clk->made;
        clk.reset();
        return fail(OXHIP_ERR_HIP, std::string("hipEventCreate: ") + hipGetErrorString(e));
    }
    return OXHIP_OK;
}

template <typename T>
static hipError_t grow(DevBuf<T>& buf, size_t count) {   // keeps a buffer that is large enough (a round reuses the last one's)
    if (buf.p && buf.n >= count) return hipSuccess;
    return buf.alloc(count ? count : 1);
}

// ------------------------------------------------------------------ the spaces
// One row per oxhip_space (kinds 0 .. OXHIP_SPACE_SE3 by index, OXHIP_SPACE_SO2 = 16 behind them: space_row): what create(), the set_* calls, setup, solve and the path entry points need to know about a space,
// as data.  A refusal text that is null means "accepted".  Adding a space = adding a row (and its launchers).
struct SpaceRow {
    uint32_t dim;               const char* bad_dim;       // the cfg.dim the space requires (0 = any), and the refusal
    uint32_t planners;          const char* bad_planner;   // bit p: built for oxhip_planner p
    const char* one_kernel;     // non-null: the space has one kernel, cfg.kernel must be OXHIP_KERNEL_AUTO / _STREAM (the refusal)
    uint32_t sphere_width;      // doubles per centre in set_spheres (0 = cfg.dim)
    const char *no_spheres, *no_boxes, *no_segments, *no_body;   // the set_* calls the space refuses
    bool radii_uploaded;        // set_spheres uploads sph_r: obstacles are compared with the radius itself
    bool goal_is_radius;        // goal_thr = the radius, compared with the space's distance (else sqrt_le_threshold(radius) against d2)
    bool midpoint_filter;       // refresh_filter runs before a solve (the space's kernels read its thresholds / grids)
    const char* no_simplify;    // simplify_paths / path_valid_matrix
    int32_t (*solve)(oxhip_rrt_batch* b);   // one launch of dp.budget iterations on b->stream
    void (*is_valid)(oxhip_rrt_batch* b, const double* states, uint32_t n, uint8_t* out);
    void (*check_motion)(oxhip_rrt_batch* b, const double* from, const double* to, uint32_t n, uint8_t* out);
};
static int32_t solve_real_vector(oxhip_rrt_batch* b);   // R^n: the planner / kernel-kind dispatch, below
static constexpr uint32_t kRrt = 1u << OXHIP_PLANNER_RRT, kConnect = 1u << OXHIP_PLANNER_RRT_CONNECT, kStar = 1u << OXHIP_PLANNER_RRT_STAR;
static const char* const kNoSegments = "segments describe the SE(2) checker";
static const char* const kNoBody = "a body describes the SE(3) checker";
static const char* const kNoSimplifySe = "simplify_paths is not built for SE(2) / SE(3) batches (their motion checks live inside their planners' kernels)";
static const char* const kSo2Arcs = "SO(2) batches take forbidden arcs (oxhip_rrt_batch_set_boxes with 1-wide rows (min, max))";
static const SpaceRow kSpaces[OXHIP_SPACE_SE3 + 2] = {
    /* OXHIP_SPACE_REAL_VECTOR */ {
        0, nullptr, kRrt | kConnect | kStar, nullptr, nullptr,
        0, nullptr, nullptr, kNoSegments, kNoBody,
        false, false, true, nullptr,
        solve_real_vector,
        [](oxhip_rrt_batch* b, const double* s, uint32_t n, uint8_t* out) { launch_is_valid(b->dp, s, n, out, b->stream); },
        [](oxhip_rrt_batch* b, const double* f, const double* t, uint32_t n, uint8_t* out) { launch_check_motion(b->dp, f, t, n, out, b->stream); }},
    /* OXHIP_SPACE_SE2 */ {
        3, "SE(2) states are (x, y, theta): dim must be 3", kConnect, "SE(2) is built for RRTConnect only", nullptr,
        0, "SE(2) batches take oxhip_rrt_batch_set_segments", "SE(2) batches take oxhip_rrt_batch_set_segments", nullptr, kNoBody,
        false, true, true, kNoSimplifySe,
        [](oxhip_rrt_batch* b) -> int32_t { launch_rrt_connect_se2(b->dp, b->stream); return OXHIP_OK; },
        [](oxhip_rrt_batch* b, const double* s, uint32_t n, uint8_t* out) { launch_se2_is_valid(b->dp, s, n, out, b->stream); },
        [](oxhip_rrt_batch* b, const double* f, const double* t, uint32_t n, uint8_t* out) { launch_se2_check_motion(b->dp, f, t, n, out, b->stream); }},
    /* OXHIP_SPACE_SO3 */ {   // cones: distance(centre, q) > radius in the SO(3) metric; rrt_so3.hip tests every cone
        4, "SO(3) states are quaternions (x, y, z, w): dim must be 4", kRrt, "SO(3) is built for RRT only",
        "SO(3) RRT runs on rrt_so3.hip: kernel must be OXHIP_KERNEL_AUTO or OXHIP_KERNEL_STREAM",
        0, nullptr, "SO(3) batches take cones (oxhip_rrt_batch_set_spheres)", kNoSegments, kNoBody,
        true, true, false, nullptr,
        [](oxhip_rrt_batch* b) -> int32_t { launch_rrt_so3(b->dp, b->stream); return OXHIP_OK; },
        [](oxhip_rrt_batch* b, const double* s, uint32_t n, uint8_t* out) { launch_so3_is_valid(b->dp, s, n, out, b->stream); },
        [](oxhip_rrt_batch* b, const double* f, const double* t, uint32_t n, uint8_t* out) { launch_so3_check_motion(b->dp, f, t, n, out, b->stream); }},
    /* OXHIP_SPACE_SE3 */ {   // world spheres with 3-wide centres, r_b + r_j against the distance; rrt_connect_se3.hip tests every sphere
        7, "SE(3) states are (x, y, z, qx, qy, qz, qw): dim must be 7", kConnect, "SE(3) is built for RRTConnect only",
        "SE(3) RRTConnect runs on rrt_connect_se3.hip: kernel must be OXHIP_KERNEL_AUTO or OXHIP_KERNEL_STREAM",
        3, nullptr, "SE(3) batches take sphere obstacles (oxhip_rrt_batch_set_spheres)", kNoSegments, nullptr,
        true, true, false, kNoSimplifySe,
        [](oxhip_rrt_batch* b) -> int32_t { launch_rrt_connect_se3(b->dp, b->obs.se3, b->stream); return OXHIP_OK; },
        [](oxhip_rrt_batch* b, const double* s, uint32_t n, uint8_t* out) { launch_se3_is_valid(b->dp, b->obs.se3, s, n, out, b->stream); },
        [](oxhip_rrt_batch* b, const double* f, const double* t, uint32_t n, uint8_t* out) { launch_se3_check_motion(b->dp, b->obs.se3, f, t, n, out, b->stream); }},
    /* OXHIP_SPACE_SO2 */ {   // arcs: min <= normalise(v) <= max, closed; rrt_so2.hip tests every arc
        1, "SO(2) states are one angle: dim must be 1", kRrt, "SO(2) is built for RRT only",
        "SO(2) RRT runs on rrt_so2.hip: kernel must be OXHIP_KERNEL_AUTO or OXHIP_KERNEL_STREAM",
        0, kSo2Arcs, nullptr, kSo2Arcs, kSo2Arcs,
        false, true, false, nullptr,
        [](oxhip_rrt_batch* b) -> int32_t { launch_rrt_so2(b->dp, b->stream); return OXHIP_OK; },
        [](oxhip_rrt_batch* b, const double* s, uint32_t n, uint8_t* out) { launch_so2_is_valid(b->dp, s, n, out, b->stream); },
        [](oxhip_rrt_batch* b, const double* f, const double* t, uint32_t n, uint8_t* out) { launch_so2_check_motion(b->dp, f, t, n, out, b->stream); }},
};
// the row of a space kind, null for an unknown one (the kinds are not contiguous: 4 .. 15 are no spaces)
static const SpaceRow* space_row(uint32_t space) {
    if (space <= OXHIP_SPACE_SE3) return &kSpaces[space];
    if (space == OXHIP_SPACE_SO2) return &kSpaces[OXHIP_SPACE_SE3 + 1];
    return nullptr;
}
static const SpaceRow& space_of(const oxhip_rrt_batch* b) { return *space_row(b->cfg.space); }   // (create() refused other kinds)

// ------------------------------------------------------------------ the entry points' shared openings
// The batch exists, setup() ran and `problem` (if one is given) is in range: what most entry points check first.  Pure host code.
static int32_t in_range(const oxhip_rrt_batch* b, int64_t problem) {
    if (problem >= (int64_t)b->cfg.n_problems) return fail(OXHIP_ERR_BAD_ARG, "problem index out of range");
    return OXHIP_OK;
}
static int32_t setup_done(const oxhip_rrt_batch* b, int64_t problem = -1) {
    if (!b) return fail(OXHIP_ERR_BAD_ARG, "null batch");
    if (!b->is_setup) return fail(OXHIP_ERR_PLANNER_UNINITIALISED, "setup() was not called");  // rrt.rs:160-163
    return in_range(b, problem);
}
// ... and the batch's device is current.  (An entry point that reports another check in between calls the steps itself, in the
// order its refusals always had.)
static int32_t ready(const oxhip_rrt_batch* b, int64_t problem = -1) {
    OX_TRY(setup_done(b, problem));
    return select_device(b->cfg.device);
}

// ------------------------------------------------------------------ create(), step by step
struct Resolved {                 // what the space's constructor makes of a config
    double fraction, res;         // the clamped lvs_fraction; res = longest valid segment length * 0.1
    double lo[OXHIP_MAX_DIM], hi[OXHIP_MAX_DIM];   // per coordinate, theta clamped to [-PI, PI]; 0 for a rotation's coordinates
    double so3_centre[4], so3_max_angle;           // SO(3) / SE(3): the rotation's bounds
};

// Every check create() makes before it chooses a device, in a fixed order (tests/golden/rrt_create_refusals.json pins order and
// texts).  Calls no HIP function.
static int32_t validate_config(const oxhip_rrt_config* cfg, Resolved& r) {
    if (cfg->struct_size != sizeof(oxhip_rrt_config)) return fail(OXHIP_ERR_BAD_ARG, "struct_size mismatch");
    if (cfg->dim == 0 || cfg->dim > OXHIP_MAX_DIM) return fail(OXHIP_ERR_BAD_ARG, "dim must be in 1..8");
    if (cfg->n_problems == 0 || cfg->max_nodes == 0) return fail(OXHIP_ERR_BAD_ARG, "n_problems and max_nodes must be > 0");
    if (cfg->max_nodes > (1u << 30)) return fail(OXHIP_ERR_BAD_ARG, "max_nodes too large");
    if (!(cfg->goal_bias >= 0.0 && cfg->goal_bias <= 1.0))
        return fail(OXHIP_ERR_BAD_ARG, "goal_bias outside [0,1] (rand Bernoulli::new would fail)");
    if (!(cfg->max_distance > 0.0) || !std::isfinite(cfg->max_distance))
        return fail(OXHIP_ERR_BAD_ARG, "max_distance must be finite and > 0");
    if (cfg->kernel > OXHIP_KERNEL_CELLS) return fail(OXHIP_ERR_BAD_ARG, "unknown kernel kind");
    if (cfg->kernel == OXHIP_KERNEL_RETIRED_3 || cfg->kernel == OXHIP_KERNEL_RETIRED_4)
        return fail(OXHIP_ERR_BAD_ARG, "kernel kinds 3 (box-pruned scan) and 4 (lane-group resolver) were retired in ABI version 2");
    if (cfg->planner > OXHIP_PLANNER_RRT_STAR) return fail(OXHIP_ERR_BAD_ARG, "unknown planner kind");
    if (cfg->frozen_split > 64) return fail(OXHIP_ERR_BAD_ARG, "frozen_split must be 0 (automatic) or 1 .. 64");
    if (cfg->kernel == OXHIP_KERNEL_CELLS && cfg->planner == OXHIP_PLANNER_RRT_CONNECT)
        return fail(OXHIP_ERR_BAD_ARG, "the cell-grid kernel runs RRT, and the geometry of the decoupled RRT*");
    if (cfg->planner == OXHIP_PLANNER_RRT_CONNECT && cfg->kernel >= OXHIP_KERNEL_RESIDENT)
        return fail(OXHIP_ERR_BAD_ARG, "RRTConnect runs on the stream kernel only");
    // RRT*: KERNEL_STREAM = rrt_star.hip (one workgroup per problem, everything in one kernel); KERNEL_LANES / KERNEL_CELLS = the
    // decoupled design (geometry by rrt_lanes.hip / rrt_cells.hip, then the wiring kernels of rrt_star_wire.hip); KERNEL_AUTO = the
    // decoupled design where it exists, its geometry by rrt_cells.hip in R^2 / R^3
    if (cfg->planner == OXHIP_PLANNER_RRT_STAR && cfg->kernel != OXHIP_KERNEL_AUTO && cfg->kernel != OXHIP_KERNEL_STREAM &&
        cfg->kernel != OXHIP_KERNEL_LANES && cfg->kernel != OXHIP_KERNEL_CELLS)
        return fail(OXHIP_ERR_BAD_ARG, "RRT* runs on the stream kernel or on the lane-per-query / cell-grid kernel + wiring kernels");
    if (cfg->planner == OXHIP_PLANNER_RRT_STAR && std::isnan(cfg->search_radius))
        return fail(OXHIP_ERR_BAD_ARG, "search_radius is NaN");
    if (cfg->goal_sampler > OXHIP_GOAL_SAMPLE_UNIFORM_DISC) return fail(OXHIP_ERR_BAD_ARG, "unknown goal sampler");
    if (cfg->goal_sampler == OXHIP_GOAL_SAMPLE_UNIFORM_DISC && (cfg->dim != 2 || cfg->space != OXHIP_SPACE_REAL_VECTOR))
        return fail(OXHIP_ERR_BAD_ARG, "the disc sampler (rrt_rvss_tests.rs:55-66) is defined for RealVectorStateSpace(2)");
    if (cfg->goal_sampler == OXHIP_GOAL_SAMPLE_UNIFORM_DISC && (cfg->planner == OXHIP_PLANNER_RRT_CONNECT || cfg->kernel == OXHIP_KERNEL_RESIDENT))
        return fail(OXHIP_ERR_BAD_ARG, "the disc sampler is built for RRT / RRT* on the stream, lane-per-query and cell-grid kernels");
    if (!space_row(cfg->space)) return fail(OXHIP_ERR_BAD_ARG, "unknown space kind");
    const SpaceRow& row = *space_row(cfg->space);
    if (row.dim != 0 && cfg->dim != row.dim) return fail(OXHIP_ERR_BAD_ARG, row.bad_dim);
    if (((row.planners >> cfg->planner) & 1u) == 0) return fail(OXHIP_ERR_BAD_ARG, row.bad_planner);
    if (row.one_kernel && cfg->kernel != OXHIP_KERNEL_AUTO && cfg->kernel != OXHIP_KERNEL_STREAM) return fail(OXHIP_ERR_BAD_ARG, row.one_kernel);
    // the bounds as the space's constructor reads them
    r = Resolved{};
    r.fraction = cfg->lvs_fraction;
    uint32_t n_box = 0;             // leading (lo, hi) pairs that bound a coordinate as given
    const double* rot = nullptr;    // (cx, cy, cz, cw, max_angle) of a rotation
    if (cfg->space == OXHIP_SPACE_SE3) {
        if (cfg->goal_sampler != OXHIP_GOAL_SAMPLE_CENTRE) return fail(OXHIP_ERR_BAD_ARG, "SE(3): the goal sampler must be OXHIP_GOAL_SAMPLE_CENTRE");
        // (x, y, z) as RealVectorStateSpace::new(3, ..); rotation bounds as SO3StateSpace::new
        OX_TRY(se_space_resolution(3, cfg->bounds, r.fraction, r.res));
        OX_TRY(so3_rotation_bounds(cfg->bounds + 6, r.so3_max_angle));
        n_box = 3; rot = cfg->bounds + 6;
    } else if (cfg->space == OXHIP_SPACE_SO3) {
        OX_TRY(so3_space_resolution(cfg->dim, cfg->bounds, r.fraction, r.res, r.so3_max_angle));   // centre, max_angle, fraction
        rot = cfg->bounds;
    } else if (cfg->space == OXHIP_SPACE_SO2) {
        OX_TRY(so2_space_resolution(cfg->bounds, r.fraction, r.res, r.lo[0], r.hi[0]));   // (lo, hi) clamped, fraction
    } else if (cfg->space == OXHIP_SPACE_SE2) {
        // SO2StateSpace::new (so2_state_space.rs:57-72): lo >= hi is InvalidBound; bounds clamped to [-PI, PI]
        const double pi = 3.14159265358979323846;
        const double th_lo = cfg->bounds[4], th_hi = cfg->bounds[5];
        if (!(th_lo < th_hi)) return fail(OXHIP_ERR_ZERO_VOLUME, "theta: lower bound >= upper bound");
        OX_TRY(se_space_resolution(2, cfg->bounds, r.fraction, r.res));
        n_box = 2;
        r.lo[2] = th_lo > -pi ? th_lo : -pi;
        r.hi[2] = th_hi < pi ? th_hi : pi;
    } else {
        OX_TRY(space_resolution(cfg->dim, cfg->bounds, r.fraction, r.res));
        n_box = cfg->dim;
    }
    if (cfg->space != OXHIP_SPACE_SO3 && cfg->max_distance / r.res > 1e6) return fail(OXHIP_ERR_BAD_ARG, "more than 1e6 validity checks per edge");
    for (uint32_t k = 0; k < n_box; ++k) { r.lo[k] = cfg->bounds[2 * k]; r.hi[k] = cfg->bounds[2 * k + 1]; }
    for (uint32_t k = 0; rot && k < 4; ++k) r.so3_centre[k] = rot[k];
    return OXHIP_OK;
}

// The batch's copy of the config and the DevParams fields that follow from cfg and Resolved alone.
static void fill_params(oxhip_rrt_batch* b, const oxhip_rrt_config* cfg, const Resolved& r) {
    b->cfg = *cfg;
    b->cfg.lvs_fraction = r.fraction;
    const uint32_t cap = ((cfg->max_nodes + 1023u) / 1024u) * 1024u;
    DevParams& dp = b->dp;
    dp.dim = cfg->dim; dp.n_problems = cfg->n_problems; dp.cap = cap; dp.max_nodes = cfg->max_nodes;
    for (uint32_t k = 0; k < cfg->dim; ++k) {
        dp.lo[k] = r.lo[k];
        dp.hi[k] = r.hi[k];
        dp.scale[k] = dp.hi[k] - dp.lo[k];
    }
    for (uint32_t k = 0; k < 4; ++k) dp.so3_centre[k] = r.so3_centre[k];
    dp.so3_max_angle = r.so3_max_angle;
    dp.space = cfg->space;
    dp.max_distance = cfg->max_distance;
    dp.res = r.res;
    if (cfg->planner == OXHIP_PLANNER_RRT_CONNECT) {   // rrt_connect.hip, rrt_connect_se2.hip: the step count of an Advanced extend's motion, when it is safely known
        const double q = cfg->max_distance / r.res, c = std::ceil(q);
        const double gap = std::fmin(q - (c - 1.0), c - q);
        if (std::isfinite(q) && c >= 1.0 && c < 4294967295.0 && gap > 1e-6) {
            dp.adv_steps = (uint32_t)c;
            dp.adv_slack = 0.5 * gap * r.res;
        }
    }
    dp.p_int = bernoulli_p_int(cfg->goal_bias);
    dp.seed = cfg->seed;
    dp.dbg_flags = cfg->debug_flags;   // oxhip_debug_flag bits: test-only, results identical (the library reads no environment variable)
    dp.goal_sampler = cfg->goal_sampler;
    dp.first_problem_id = cfg->first_problem_id;
    dp.stop_at_goal = cfg->stop_at_goal ? 1 : 0;
    dp.t_steer = sqrt_le_threshold(cfg->max_distance);
    dp.thr_search = sqrt_lt_threshold(cfg->search_radius);
}

// RRT*'s buffers (Star), for the decoupled design (Star::Wiring, `on`) or the one-kernel design; KERNEL_AUTO falls back from the
// first to the second when the first's memory is not to be had.  `e` collects the first failure, as in alloc_common, which binds
// what this allocates.
static int32_t alloc_star(oxhip_rrt_batch* b, hipError_t& e) {
    const oxhip_rrt_config* cfg = &b->cfg;
    DevParams& dp = b->dp;
    Star::Wiring& w = b->star.wiring;
    const uint32_t P = cfg->n_problems, dim = cfg->dim, cap = dp.cap;
    auto chk = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    const bool geo_cells = cfg->kernel != OXHIP_KERNEL_LANES && cells_supported(dim, cap);
    const bool geo_lanes = cfg->kernel != OXHIP_KERNEL_CELLS && lanes_supported(dim, cap);
    const bool can_wire = star_wire_supported(dim) && (geo_cells || geo_lanes);
    w.on = cfg->kernel == OXHIP_KERNEL_LANES || cfg->kernel == OXHIP_KERNEL_CELLS || (cfg->kernel == OXHIP_KERNEL_AUTO && can_wire);
    if (w.on && !can_wire) return fail(OXHIP_ERR_BAD_ARG, "decoupled RRT*: neither geometry kernel supports this (dim, max_nodes)");
    w.geo_cells = w.on && geo_cells;
    chk(b->star.cost.alloc((size_t)P * cap));
    chk(b->star.wire_chk.alloc(P));
    if (w.on && e == hipSuccess) {
        // neighbour lists: a pool segment per problem; a round wires the longest prefix of a problem's pending nodes whose
        // lists fit (mean list length at radius 1 in configs[1]'s world: ~40), so the size bounds memory, not the result.
        // Footprint per problem: share x 16 B of pool + (share / 32 + cap) x 144 B of chunk store + 4 x cap x 4..8 B; the
        // default share is 64 x cap, cut so that pool + chunks of the whole batch stay below 24 GB.
        uint64_t share = 64ull * cap;
        const uint64_t budget_entries = (24ull << 30) / (sizeof(StarEntry) + sizeof(StarChunk) / 32) / P;
        if (share > budget_entries) share = budget_entries;
        if (cfg->star_pool_share != 0 && cfg->star_pool_share < share) share = cfg->star_pool_share;
        if (share < cap) share = cap;   // a single list is at most cap entries long: every round wires at least one node
        dp.pool_share = (uint32_t)share;
        hipError_t ew = hipSuccess;
        auto chkw = [&](hipError_t r) { if (ew == hipSuccess) ew = r; };
        chkw(w.stream2.take(cfg->device));
        for (auto& ev : w.ev_seg) chkw(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        chkw(hipEventCreateWithFlags(&w.ev_join, hipEventDisableTiming));
        chkw(w.pool.alloc((size_t)P * share + 64));   // (+ padding: masked lanes of the wiring kernel read one entry past an empty list)
        dp.chunk_share = (uint32_t)(share / 32 + cap);   // enough for any set of lists that fits the pool segment (one partial chunk per node)
        chkw(w.chunks.alloc((size_t)P * dp.chunk_share));
        chkw(w.chunk_cursor.alloc(P));
        chkw(w.wired.alloc(P));
        chkw(w.nbr_take.alloc(P));
        chkw(w.nbr_total.alloc(P));
        chkw(w.nbr_cnt.alloc((size_t)P * cap));
        chkw(w.nbr_off.alloc((size_t)P * cap));
        chkw(w.d_near.alloc((size_t)P * cap));
        if (ew != hipSuccess && cfg->kernel == OXHIP_KERNEL_AUTO) {
            // KERNEL_AUTO promised "whatever runs": the one-kernel design (rrt_star.hip) needs 1/60 of this memory
            (void)hipGetLastError();
            w.release();
            dp.pool_share = dp.chunk_share = 0;
            w.on = false;
            w.geo_cells = false;
        } else {
            chk(ew);
        }
    }
    if (!w.on) {
        chk(b->star.nb_idx.alloc((size_t)P * cap));
        chk(b->star.nb_dist.alloc((size_t)P * cap));
    }
    return OXHIP_OK;
}

// The stream, the solve clock's events and the buffers every batch has (the planner's own among them, RRT*'s by alloc_star at the
// place its allocations always had), then the binds of the parts they belong to.
static int32_t alloc_common(oxhip_rrt_batch* b) {
    const oxhip_rrt_config* cfg = &b->cfg;
    const uint32_t P = cfg->n_problems, dim = cfg->dim, cap = b->dp.cap;
    hipError_t e = hipSuccess;
    auto chk = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    chk(b->stream.take(cfg->device));
    chk(b->solve.clk.made);   // an event that could not be made refuses the create, as a buffer does
    chk(b->trees.tree.alloc((size_t)P * dim * cap));
    chk(b->trees.parent.alloc((size_t)P * cap));
    chk(b->trees.skip.alloc((size_t)P * cap));
    if (cfg->planner == OXHIP_PLANNER_RRT_CONNECT) {
        chk(b->trees.tree_b.alloc((size_t)P * dim * cap));
        chk(b->trees.parent_b.alloc((size_t)P * cap));
    }
    if (cfg->planner == OXHIP_PLANNER_RRT_STAR) OX_TRY(alloc_star(b, e));
    chk(b->trees.state.alloc(P));
    chk(b->goals.goal_c.alloc((size_t)P * dim));
    chk(b->goals.goal_thr.alloc(P));
    chk(b->goals.goal_r.alloc(P));
    if (!space_of(b).no_body && e == hipSuccess) {   // the default body: one sphere of radius 0 at the origin (a point)
        if (upload(b->obs.se3_body, std::vector<double>(4 * (size_t)kSe3MaxBody, 0.0), b->stream) != OXHIP_OK) e = hipErrorOutOfMemory;
        b->obs.se3.n_body = 1;
    }
    if (e != hipSuccess) return alloc_failed(e);
    b->trees.bind(b->dp); b->goals.bind(b->dp); b->star.bind(b->dp); b->obs.bind(b->dp);
    return OXHIP_OK;
}

// rrt_cells.hip's arena (the comment at Cells) and the DevParams fields that describe it.
static int32_t alloc_cells(oxhip_rrt_batch* b) {
    DevParams& dp = b->dp;
    Cells& c = b->cells;
    const uint32_t P = b->cfg.n_problems, dim = b->cfg.dim, cap = dp.cap;
    dp.cell_level_max = cells_level_max(dim, cap);
    // head blocks for the finest grid this capacity reaches + the overflow blocks (n nodes overflow into at most n / 7)
    dp.cell_blocks = cells_head_blocks(dim, cap) + cap / 7u + 64u;
    // frozen launches: a problem's iterations are independent, so they are divided over enough waves to fill the chip
    // (256 CUs x 12 waves of the frozen specialisation's register budget)
    uint32_t split = b->cfg.frozen_split;
    if (split == 0) { split = (3072u + P - 1u) / P; if (split > 8u) split = 8u; if (split < 1u) split = 1u; }
    dp.cells_split = split;
    dp.sph_grid_G = sphere_grid_side(dim);
    const size_t grid_cells = dim == 2 ? (size_t)dp.sph_grid_G * dp.sph_grid_G : (size_t)dp.sph_grid_G * dp.sph_grid_G * dp.sph_grid_G;
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t at = off; off = (off + bytes + 255u) & ~(size_t)255u; return at; };
    const size_t o_meta = carve((size_t)P * sizeof(CellMeta)), o_acc = carve((size_t)P * sizeof(CellAcc));   // (zeroed together)
    const size_t o_board = carve(2 * kCellsBoardWords * sizeof(uint64_t));   // the frozen launches' progress boards: zero before the first
    const size_t zero_bytes = off;
    const size_t o_pos = carve((size_t)P * 64 * sizeof(uint64_t)), o_grid = carve(grid_cells * sizeof(uint64_t));
    const size_t o_grid2 = carve(b->star.wiring.on ? grid_cells * sizeof(uint64_t) : 0);
    const size_t o_flat = carve((size_t)P * 4096 * 4 * sizeof(float)), o_xyz = carve((size_t)P * cap * 4 * sizeof(double));
    const size_t o_blk = carve((size_t)P * dp.cell_blocks * sizeof(CellBlock));
    hipError_t e = c.arena.alloc(off);
    if (e == hipSuccess) e = hipMemset(c.arena.p, 0, zero_bytes);
    if (e != hipSuccess) return alloc_failed(e);
    uint8_t* base = c.arena.p;
    c.meta = reinterpret_cast<CellMeta*>(base + o_meta);
    c.sph_grid = reinterpret_cast<uint64_t*>(base + o_grid);
    if (b->star.wiring.on) c.star_grid = reinterpret_cast<uint64_t*>(base + o_grid2);
    dp.cell_blk = reinterpret_cast<CellBlock*>(base + o_blk); dp.cell_flat = reinterpret_cast<float*>(base + o_flat);
    dp.cell_xyz = reinterpret_cast<double*>(base + o_xyz); dp.cell_meta = c.meta;
    dp.cell_acc = reinterpret_cast<CellAcc*>(base + o_acc); dp.cell_part_pos = reinterpret_cast<uint64_t*>(base + o_pos);
    dp.sph_grid = c.sph_grid;
    dp.cell_board = reinterpret_cast<uint64_t*>(base + o_board);
    dp.cells_parity = 0;
    return OXHIP_OK;
}

// R^n's streaming kernels (rrt_stream.hip; RRT*: star_shadow's) screen their scans over an fl32 shadow of the tree, which they
// maintain themselves.
static int32_t alloc_shadow(oxhip_rrt_batch* b) {
    const size_t P = b->cfg.n_problems;
    hipError_t e = b->shadow.tree32.alloc(P * b->cfg.dim * b->dp.cap);
    if (e == hipSuccess) e = b->shadow.state.alloc(P * 2);
    if (e == hipSuccess) e = hipMemset(b->shadow.state.p, 0, P * 2 * sizeof(uint32_t));
    if (e != hipSuccess) return alloc_failed(e);
    b->shadow.bind(b->dp);
    return OXHIP_OK;
}

// ------------------------------------------------------------------ the stand-alone primitives' shared body
// The body of the element-wise primitives: rows of w_a / w_b / w_out doubles for a / b / out, one double per row of t; b and t
// travel only when the op reads them.  launch(a, b, t, out, stream) on device pointers.
template <typename Launch>
static int32_t op_batch(int32_t device, const double* a, const double* b, const double* t, uint32_t n, double* out,
                        size_t w_a, size_t w_b, size_t w_out, bool b_uploaded, bool t_uploaded, Launch launch) {
    if (n == 0) return OXHIP_OK;
    OX_TRY(select_device(device));
    PooledStream ts;
    OX_TRY(ts.acquire(device));
    DevBuf<double> da, db, dt, dout;
    OX_TRY(to_device(da, a, w_a * n, ts.s));
    if (b_uploaded) OX_TRY(to_device(db, b, w_b * n, ts.s));
    if (t_uploaded) OX_TRY(to_device(dt, t, n, ts.s));
    HIP_TRY(dout.alloc(w_out * n));
    launch(da.p, db.p, dt.p, dout.p, ts.s);
    HIP_TRY(hipGetLastError());
    return to_host(out, dout, w_out * n, ts.s);
}

extern "C" {

int32_t oxhip_abi_version(void) { return OXHIP_ABI_VERSION; }

const char* oxhip_status_string(int32_t s) {
    switch (s) {
        case OXHIP_OK: return "ok";
        case OXHIP_ERR_TIMEOUT: return "No solution found within timeout.";  // Display strings of error.rs:110-136
        case OXHIP_ERR_NO_SOLUTION_FOUND: return "No solution found.";
        case OXHIP_ERR_PLANNER_UNINITIALISED: return "<Planner>.setup() was not called, thus Planner is uninitialised.";
        case OXHIP_ERR_INVALID_START_STATE: return "Start state is not valid in the current StateSpace.";
        case OXHIP_ERR_UNSAMPLED_STATE_SPACE: return "StateSpace is not sampled. Either Tree or Roadmap is empty.";
        case OXHIP_ERR_BAD_ARG: return "bad argument";
        case OXHIP_ERR_UNBOUNDED: return "Cannot sample uniformly because a dimension is unbounded.";
        case OXHIP_ERR_ZERO_VOLUME: return "Cannot sample from a region with zero volume.";
        case OXHIP_ERR_CAPACITY: return "caller buffer too small";
        case OXHIP_ERR_HIP: return "HIP runtime error";
        case OXHIP_ERR_NO_DEVICE: return "no HIP device (no CPU fallback exists)";
        default: return "unknown status";
    }
}

const char* oxhip_last_error_string(void) { return g_last_error.c_str(); }

int32_t oxhip_device_count(int32_t* count) {
    if (!count) return fail(OXHIP_ERR_BAD_ARG, "count is null");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    *count = (e == hipSuccess) ? c : 0;
    if (e != hipSuccess || c <= 0) return fail(OXHIP_ERR_NO_DEVICE, "no HIP device visible");
    return OXHIP_OK;
}

int32_t oxhip_rrt_batch_create(const oxhip_rrt_config* cfg, oxhip_rrt_batch** out) {
    if (!cfg || !out) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    *out = nullptr;
    Resolved r;
    OX_TRY(validate_config(cfg, r));
    OX_TRY(select_device(cfg->device));
    // from here on every early return destroys the batch, and with it whatever it took so far
    std::unique_ptr<oxhip_rrt_batch, decltype(&oxhip_rrt_batch_destroy)> b(new oxhip_rrt_batch(), oxhip_rrt_batch_destroy);
    fill_params(b.get(), cfg, r);
    OX_TRY(alloc_common(b.get()));
    const uint32_t dim = cfg->dim, cap = b->dp.cap;
    uint32_t kind = cfg->kernel;
    if (space_of(b.get()).one_kernel) kind = OXHIP_KERNEL_STREAM;   // (e.g. rrt_so3.hip: the space's one kernel, reported as the streaming kind)
    if (cfg->planner != OXHIP_PLANNER_RRT) kind = b->star.wiring.on ? (b->star.wiring.geo_cells ? OXHIP_KERNEL_CELLS : OXHIP_KERNEL_LANES) : OXHIP_KERNEL_STREAM;
    if (kind == OXHIP_KERNEL_AUTO) {
        // rrt_cells.hip (one wave per problem, R^2 / R^3, trees up to 64,512 nodes) wherever it exists: since its rounds
        // repair overtaken queries in place it grows ONE tree to 10,000 nodes in 4.3 ms -- faster than rrt_lanes.hip, which gives
        // the problem a whole CU (5.6 ms) -- and 256 of them in 4.9 ms (6.2 ms), profiles/r3_single/.  rrt_lanes.hip serves
        // R^4 .. R^6 (and trees that fit its register rows), rrt_stream.hip everything else.
        kind = cells_supported(dim, cap) ? OXHIP_KERNEL_CELLS : lanes_supported(dim, cap) ? OXHIP_KERNEL_LANES : OXHIP_KERNEL_STREAM;
    }
    if (kind == OXHIP_KERNEL_CELLS && !cells_supported(dim, cap))
        return fail(OXHIP_ERR_BAD_ARG, "cell-grid kernel: R^2 / R^3 trees of at most 64,512 nodes");
    if (kind == OXHIP_KERNEL_LANES && !lanes_supported(dim, cap))
        return fail(OXHIP_ERR_BAD_ARG, "resident (lane-per-query) kernel does not support this (dim, max_nodes)");
    if (kind == OXHIP_KERNEL_RESIDENT && !resident_supported(dim, cap))
        return fail(OXHIP_ERR_BAD_ARG, "resident kernel does not support this (dim, max_nodes)");
    b->solve.kernel_kind = kind;
    if (kind == OXHIP_KERNEL_CELLS) OX_TRY(alloc_cells(b.get()));
    // (a space with a kernel of its own keeps no shadow; RRT* does on every kind)
    if ((cfg->planner == OXHIP_PLANNER_RRT && kind == OXHIP_KERNEL_STREAM && !space_of(b.get()).one_kernel) || cfg->planner == OXHIP_PLANNER_RRT_STAR)
        OX_TRY(alloc_shadow(b.get()));
    *out = b.release();
    return OXHIP_OK;
}

int32_t oxhip_rrt_batch_destroy(oxhip_rrt_batch* b) {
    if (!b) return OXHIP_OK;
    (void)hipSetDevice(b->cfg.device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    delete b;   // (the order of what goes: the comment at oxhip_rrt_batch)
    return OXHIP_OK;
}

int32_t oxhip_rrt_batch_set_spheres(oxhip_rrt_batch* b, const double* centres, const double* radii, uint32_t n) {
    if (!b || (n && (!centres || !radii))) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    const SpaceRow& row = space_of(b);
    if (row.no_spheres) return fail(OXHIP_ERR_BAD_ARG, row.no_spheres);
    OX_TRY(select_device(b->cfg.device));
    const uint32_t dim = row.sphere_width ? row.sphere_width : b->cfg.dim;
    std::vector<double> c((size_t)dim * n), thr(n);
    for (uint32_t j = 0; j < n; ++j) {
        for (uint32_t k = 0; k < dim; ++k) {
            double v = centres[(size_t)j * dim + k];
            if (!(std::fabs(v) <= kMaxMagnitude)) return fail(OXHIP_ERR_BAD_ARG, "sphere centre not finite / too large");
            c[(size_t)k * n + j] = v;  // SoA [dim][n]
        }
        thr[j] = sqrt_le_threshold(radii[j]);
    }
    Obstacles& o = b->obs;
    OX_TRY(upload(o.sph_c, c, b->stream));
    OX_TRY(upload(o.sph_thr, thr, b->stream));
    o.n_spheres = n;
    o.bind(b->dp);
    o.sph_centres.assign(centres, centres + (size_t)n * dim);
    o.sph_radii.assign(radii, radii + n);
    o.filt_dirty = o.radii_dirty = true;
    if (row.radii_uploaded) OX_TRY(upload_radii(b));
    return OXHIP_OK;
}

int32_t oxhip_rrt_batch_set_boxes(oxhip_rrt_batch* b, const double* lo, const double* hi, uint32_t n) {
    if (!b || (n && (!lo || !hi))) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    if (space_of(b).no_boxes) return fail(OXHIP_ERR_BAD_ARG, space_of(b).no_boxes);
    OX_TRY(select_device(b->cfg.device));
    const uint32_t dim = b->cfg.dim;
    std::vector<double> l((size_t)dim * n), h((size_t)dim * n);
    for (uint32_t j = 0; j < n; ++j)
        for (uint32_t k = 0; k < dim; ++k) {
            l[(size_t)k * n + j] = lo[(size_t)j * dim + k];
            h[(size_t)k * n + j] = hi[(size_t)j * dim + k];
        }
    OX_TRY(upload(b->obs.box_lo, l, b->stream));
    OX_TRY(upload(b->obs.box_hi, h, b->stream));
    b->obs.n_boxes = n;
    b->obs.bind(b->dp);
    return OXHIP_OK;
}

int32_t oxhip_rrt_batch_set_segments(oxhip_rrt_batch* b, const double* segments, uint32_t n, double clearance) {
    if (!b || (n && !segments)) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    if (space_of(b).no_segments) return fail(OXHIP_ERR_BAD_ARG, space_of(b).no_segments);
    if (std::isnan(clearance)) return fail(OXHIP_ERR_BAD_ARG, "clearance is NaN");
    OX_TRY(select_device(b->cfg.device));
    std::vector<double> v(segments, segments + (size_t)4 * n);
    for (double x : v) if (!(std::fabs(x) <= kMaxMagnitude)) return fail(OXHIP_ERR_BAD_ARG, "segment endpoint not finite / too large");
    OX_TRY(upload(b->obs.segs, v, b->stream));
    b->obs.n_segs = n;
    b->obs.bind(b->dp);
    b->dp.seg_thr = sqrt_le_threshold(clearance);
    // the grid the motion check looks its segments up in: over the (x, y) bounds, which are finite here (create() refused others)
    b->dp.seg_grid = nullptr;
    const double wx = b->dp.hi[0] - b->dp.lo[0], wy = b->dp.hi[1] - b->dp.lo[1];
    if (n > 0 && (b->cfg.debug_flags & OXHIP_DEBUG_SE2_NO_SEGMENT_GRID) == 0 && std::isfinite(wx) && std::isfinite(wy) && wx > 0.0 && wy > 0.0) {
        const uint32_t G = seg_grid_side();
        if (b->obs.seg_grid.n != (size_t)G * G * 8) HIP_TRY(b->obs.seg_grid.alloc((size_t)G * G * 8));
        b->dp.seg_grid_G = G;
        b->dp.seg_grid_inv[0] = (double)G / wx;
        b->dp.seg_grid_inv[1] = (double)G / wy;
        launch_seg_grid(b->dp, b->obs.seg_grid.p, clearance, b->stream);
        b->dp.seg_grid = b->obs.seg_grid.p;
    }
    return OXHIP_OK;
}

int32_t oxhip_rrt_batch_set_body(oxhip_rrt_batch* b, const double* centres, const double* radii, uint32_t n) {
    if (!b || !centres || !radii) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    if (space_of(b).no_body) return fail(OXHIP_ERR_BAD_ARG, space_of(b).no_body);
    if (n == 0 || n > (uint32_t)kSe3MaxBody) return fail(OXHIP_ERR_BAD_ARG, "a body has 1 .. 16 spheres");
    std::vector<double> v(4 * (size_t)kSe3MaxBody, 0.0);   // SoA [4][kSe3MaxBody]
    for (uint32_t j = 0; j < n; ++j) {
        for (uint32_t k = 0; k < 3; ++k) {
            const double c = centres[(size_t)j * 3 + k];
            if (!(std::fabs(c) <= kMaxMagnitude)) return fail(OXHIP_ERR_BAD_ARG, "body sphere centre not finite / too large");
            v[(size_t)k * kSe3MaxBody + j] = c;
        }
        if (!(radii[j] >= 0.0 && radii[j] <= kMaxMagnitude)) return fail(OXHIP_ERR_BAD_ARG, "body sphere radius must be finite and >= 0");
        v[3 * (size_t)kSe3MaxBody + j] = radii[j];
    }
    OX_TRY(select_device(b->cfg.device));
    OX_TRY(upload(b->obs.se3_body, v, b->stream));
    b->obs.se3.n_body = n;
    b->obs.bind(b->dp);
    return OXHIP_OK;
}

int32_t oxhip_rrt_batch_setup(oxhip_rrt_batch* b, const double* starts, const double* goal_centres,
                              const double* goal_radii) {
    if (!b || !starts || !goal_centres || !goal_radii) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    drop_derived(b);
    OX_TRY(select_device(b->cfg.device));
    const uint32_t P = b->cfg.n_problems, dim = b->cfg.dim, cap = b->dp.cap;
    for (size_t i = 0; i < (size_t)P * dim; ++i)
        if (!(std::fabs(starts[i]) <= kMaxMagnitude) || !(std::fabs(goal_centres[i]) <= kMaxMagnitude))
            return fail(OXHIP_ERR_BAD_ARG, "start / goal centre not finite or beyond 1e150");
    if (b->cfg.goal_sampler == OXHIP_GOAL_SAMPLE_UNIFORM_DISC)
        for (uint32_t p = 0; p < P; ++p)
            if (!(goal_radii[p] >= 0.0 && goal_radii[p] <= kMaxMagnitude)) return fail(OXHIP_ERR_BAD_ARG, "disc sampler: goal radius must be finite and >= 0");
    b->goals.starts.assign(starts, starts + (size_t)P * dim);
    b->obs.filt_dirty = true;
    std::vector<double> thr(P);
    // R^n: satisfied iff d2 <= T(radius); SE(2) / SO(3) / SE(3): the space's distance is compared with the radius itself
    for (uint32_t p = 0; p < P; ++p) thr[p] = space_of(b).goal_is_radius ? goal_radii[p] : sqrt_le_threshold(goal_radii[p]);
    std::vector<ProblemState> states(P);
    for (auto& s : states) {
        s = ProblemState{};
        s.checksum = kFnvBasis;
        s.n_nodes = 1;
        s.goal_node = -1;
        s.goal_node_b = -1;
        s.n_nodes_b = b->cfg.planner == OXHIP_PLANNER_RRT_CONNECT ? 1 : 0;
        s.stop_reason = OXHIP_STOP_NONE;
    }
    std::vector<int32_t> root(1, -1);
    Trees& t = b->trees;
    HIP_TRY(hipMemcpyAsync(b->goals.goal_c.p, goal_centres, (size_t)P * dim * sizeof(double), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(b->goals.goal_thr.p, thr.data(), P * sizeof(double), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(b->goals.goal_r.p, goal_radii, P * sizeof(double), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(t.state.p, states.data(), P * sizeof(ProblemState), hipMemcpyHostToDevice, b->stream));
    // tree.clear(); tree.push(Node{start_states[0], None})   rrt.rs:147-155
    // node 0 of coordinate k of problem p lives at tree[(p*dim + k)*cap]: strided 2-D copy
    HIP_TRY(hipMemcpy2DAsync(t.tree.p, (size_t)cap * sizeof(double), starts, sizeof(double), sizeof(double),
                             (size_t)P * dim, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemsetAsync(t.skip.p, 0, (size_t)P * cap, b->stream));
    OX_TRY(reset_tree_caches(b, 0, P));
    std::vector<int32_t> minus1(P, -1);
    HIP_TRY(hipMemcpy2DAsync(t.parent.p, (size_t)cap * sizeof(int32_t), minus1.data(), sizeof(int32_t),
                             sizeof(int32_t), P, hipMemcpyHostToDevice, b->stream));
    if (b->cfg.planner == OXHIP_PLANNER_RRT_CONNECT) {
        // goal_tree.push(Node{goal.sample_goal(), None})  rrt_connect.rs:218-224 (the ball goal samples its centre)
        HIP_TRY(hipMemcpy2DAsync(t.tree_b.p, (size_t)cap * sizeof(double), goal_centres, sizeof(double), sizeof(double),
                                 (size_t)P * dim, hipMemcpyHostToDevice, b->stream));
        HIP_TRY(hipMemcpy2DAsync(t.parent_b.p, (size_t)cap * sizeof(int32_t), minus1.data(), sizeof(int32_t),
                                 sizeof(int32_t), P, hipMemcpyHostToDevice, b->stream));
    }
    if (b->cfg.planner == OXHIP_PLANNER_RRT_STAR) {   // start node: cost 0.0 (rrt_star.rs:163-167)
        HIP_TRY(hipMemsetAsync(b->star.cost.p, 0, (size_t)P * cap * sizeof(double), b->stream));
        HIP_TRY(hipMemsetAsync(b->star.wire_chk.p, 0, (size_t)P * sizeof(uint64_t), b->stream));
        if (b->star.wiring.on) {
            std::vector<uint32_t> one(P, 1u);   // the start node needs no wiring
            HIP_TRY(hipMemcpyAsync(b->star.wiring.wired.p, one.data(), (size_t)P * sizeof(uint32_t), hipMemcpyHostToDevice, b->stream));
            HIP_TRY(hipStreamSynchronize(b->stream));
        }
    }
    HIP_TRY(hipStreamSynchronize(b->stream));
    b->is_setup = true;
    return OXHIP_OK;
}

// ---- the filters a launch reads (the thresholds' arithmetic: oxhip_host.hpp), each built under its own condition by refresh_filter
// rrt_connect.hip's motion check looks a state's spheres up (R^2 / R^3, up to 64 spheres, finite bounds): bit j of a cell's
// mask = sphere j reaches the cell's box (sphere_grid_kernel: squared distance centre - box, the box taken 2^-9 of a cell
// wider, compared with connect_grid_threshold).
static int32_t connect_sphere_grid(oxhip_rrt_batch* b) {
    Obstacles& o = b->obs;
    const uint32_t n = o.n_spheres, dim = b->cfg.dim;
    b->dp.sph_grid = nullptr;
    bool ok = (dim == 2 || dim == 3) && n >= 1 && n <= 64 && (b->cfg.debug_flags & OXHIP_DEBUG_SE2_NO_SEGMENT_GRID) == 0;
    for (uint32_t k = 0; ok && k < dim; ++k) ok = std::isfinite(b->dp.lo[k]) && std::isfinite(b->dp.hi[k]) && b->dp.hi[k] > b->dp.lo[k];
    if (!ok) return OXHIP_OK;
    const uint32_t G = sphere_grid_side(dim);
    const size_t cells = dim == 2 ? (size_t)G * G : (size_t)G * G * G;
    if (o.conn_grid.n != cells) HIP_TRY(o.conn_grid.alloc(cells));
    std::vector<double> f(n);
    for (uint32_t j = 0; j < n; ++j) f[j] = connect_grid_threshold(o.sph_radii[j]);
    OX_TRY(upload(o.conn_filt, f, b->stream));
    b->dp.sph_grid_G = G;
    launch_sphere_grid(b->dp, o.conn_grid.p, o.conn_filt.p, b->stream);
    b->dp.sph_grid = o.conn_grid.p;
    return OXHIP_OK;
}
// The midpoint filter of a planner's motion check (midpoint_threshold, h for a motion of max_distance), and rrt_cells.hip's grid
// of it.
static int32_t midpoint_filter(oxhip_rrt_batch* b, double maxabs) {
    Obstacles& o = b->obs;
    const uint32_t n = o.n_spheres;
    const double h = 0.5 * b->cfg.max_distance * (1.0 + 1e-6) + 1e-9 * maxabs;
    std::vector<double> f(n);
    for (uint32_t j = 0; j < n; ++j) f[j] = midpoint_threshold(o.sph_radii[j], h);
    OX_TRY(upload(o.sph_filt, f, b->stream));
    o.bind(b->dp);
    if (b->cells.sph_grid && n > 0) launch_sphere_grid(b->dp, b->cells.sph_grid, o.sph_filt.p, b->stream);   // (rrt_cells.hip looks the midpoint filter up)
    return OXHIP_OK;
}
// Decoupled RRT*: motion_seq.hpp filters motions of any length, so it takes the radii as given and the absolute margin; the edge
// kernel's grid is built for motions up to search_radius long (star_edge_threshold).
static int32_t star_edge_filter(oxhip_rrt_batch* b, double maxabs) {
    Obstacles& o = b->obs;
    const uint32_t n = o.n_spheres;
    OX_TRY(upload_radii(b));
    b->dp.filt_abs = 1e-9 * maxabs;
    b->dp.star_sph_grid = nullptr;
    if (!b->cells.star_grid || n == 0) return OXHIP_OK;
    const double h_lo = b->dp.filt_abs, h_hi = 0.5 * b->cfg.search_radius * (1.0 + 1e-6) + b->dp.filt_abs;
    std::vector<double> sf(n);
    for (uint32_t j = 0; j < n; ++j) sf[j] = star_edge_threshold(o.sph_radii[j], h_lo, h_hi);
    OX_TRY(upload(b->star.wiring.star_filt, sf, b->stream));
    launch_sphere_grid(b->dp, b->cells.star_grid, b->star.wiring.star_filt.p, b->stream);
    b->dp.star_sph_grid = b->cells.star_grid;
    return OXHIP_OK;
}
// Before a launch of a space whose kernels read them (SpaceRow::midpoint_filter): whatever spheres, starts or bounds changed.
static int32_t refresh_filter(oxhip_rrt_batch* b) {
    if (!b->obs.filt_dirty) return OXHIP_OK;
    if (b->cfg.planner == OXHIP_PLANNER_RRT_CONNECT && b->cfg.space == OXHIP_SPACE_REAL_VECTOR) {
        OX_TRY(connect_sphere_grid(b));
    } else {
        const double maxabs = filter_maxabs(b->cfg, b->obs.sph_centres, &b->goals.starts);
        OX_TRY(midpoint_filter(b, maxabs));
        if (b->star.wiring.on) OX_TRY(star_edge_filter(b, maxabs));
    }
    b->obs.filt_dirty = false;
    return OXHIP_OK;
}

static int32_t read_states(oxhip_rrt_batch* b, std::vector<ProblemState>& states) {
    Trees& t = b->trees;
    states.resize(b->cfg.n_problems);
    if (!t.h_states) HIP_TRY(hipHostMalloc((void**)&t.h_states, states.size() * sizeof(ProblemState), hipHostMallocDefault));
    HIP_TRY(hipMemcpyAsync(t.h_states, t.state.p, states.size() * sizeof(ProblemState), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    std::memcpy(states.data(), t.h_states, states.size() * sizeof(ProblemState));
    return OXHIP_OK;
}

int32_t oxhip_rrt_batch_set_tree(oxhip_rrt_batch* b, uint32_t problem, const double* states_in, const int32_t* parents_in,
                                 uint32_t n) {
    if (!b || !states_in || !parents_in) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    drop_derived(b);
    OX_TRY(setup_done(b, problem));
    if (n == 0 || n > b->cfg.max_nodes) return fail(OXHIP_ERR_BAD_ARG, "n_nodes must be in 1..max_nodes");
    if (b->cfg.planner != OXHIP_PLANNER_RRT) return fail(OXHIP_ERR_BAD_ARG, "set_tree is for the RRT planner");
    OX_TRY(select_device(b->cfg.device));
    const uint32_t dim = b->cfg.dim, cap = b->dp.cap;
    if (parents_in[0] != -1) return fail(OXHIP_ERR_BAD_ARG, "parents[0] must be -1 (the root)");
    std::vector<double> soa((size_t)dim * n);
    std::vector<uint8_t> skip(n, 0);
    for (uint32_t i = 0; i < n; ++i) {
        if (i > 0 && (parents_in[i] < 0 || (uint32_t)parents_in[i] >= i)) return fail(OXHIP_ERR_BAD_ARG, "parent index must precede its child");
        for (uint32_t k = 0; k < dim; ++k) {
            double v = states_in[(size_t)i * dim + k];
            if (!(std::fabs(v) <= kMaxMagnitude)) return fail(OXHIP_ERR_BAD_ARG, "state not finite or beyond 1e150");
            soa[(size_t)k * n + i] = v;
        }
    }
    // skip flag: a node whose coordinates equal (as values) those of a lower-index node can never be nearest
    {
        std::vector<uint32_t> order(n);
        for (uint32_t i = 0; i < n; ++i) order[i] = i;
        auto key_less = [&](uint32_t a, uint32_t c) {
            for (uint32_t k = 0; k < dim; ++k) {
                double x = soa[(size_t)k * n + a] + 0.0, y = soa[(size_t)k * n + c] + 0.0;  // -0.0 -> +0.0
                if (x < y) return true;
                if (y < x) return false;
            }
            return a < c;
        };
        std::sort(order.begin(), order.end(), key_less);
        for (uint32_t j = 1; j < n; ++j) {
            bool same = true;
            for (uint32_t k = 0; k < dim && same; ++k) same = soa[(size_t)k * n + order[j]] == soa[(size_t)k * n + order[j - 1]];
            if (same) skip[order[j]] = 1;  // order[j-1] has the lower index among equals (ties sort by index)
        }
    }
    HIP_TRY(hipMemcpy2DAsync(b->trees.tree.p + (size_t)problem * dim * cap, (size_t)cap * sizeof(double), soa.data(),
                             (size_t)n * sizeof(double), (size_t)n * sizeof(double), dim, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(b->trees.parent.p + (size_t)problem * cap, parents_in, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(b->trees.skip.p + (size_t)problem * cap, skip.data(), n, hipMemcpyHostToDevice, b->stream));
    OX_TRY(reset_tree_caches(b, problem, 1));
    std::vector<ProblemState> states;
    OX_TRY(read_states(b, states));
    states[problem].n_nodes = n;
    HIP_TRY(hipMemcpyAsync(b->trees.state.p + problem, &states[problem], sizeof(ProblemState), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return OXHIP_OK;
}

// Decoupled RRT*: parents and costs of the nodes the RRT kernel just inserted (rrt_star_wire.hip).  A round wires, per
// problem, the longest prefix of its pending nodes whose neighbour lists fit the problem's pool segment; usually one round.
static int32_t wire_new_nodes(oxhip_rrt_batch* b) {
    Star::Wiring& w = b->star.wiring;
    const uint32_t P = b->cfg.n_problems;
    std::vector<ProblemState> states;
    std::vector<uint32_t> wired(P), take(P), total(P), chunks_used(P);
    for (;;) {
        OX_TRY(read_states(b, states));
        HIP_TRY(hipMemcpyAsync(wired.data(), w.wired.p, (size_t)P * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
        uint32_t max_pending = 0;
        for (uint32_t p = 0; p < P; ++p) {
            const uint32_t pend = states[p].n_nodes > wired[p] ? states[p].n_nodes - wired[p] : 0u;
            max_pending = pend > max_pending ? pend : max_pending;
        }
        if (max_pending == 0) return OXHIP_OK;
        uint32_t max_n = 0;
        for (uint32_t p = 0; p < P; ++p) max_n = states[p].n_nodes > max_n ? states[p].n_nodes : max_n;
        launch_star_shadow(b->dp, max_n, b->stream);
        HIP_TRY(hipMemsetAsync(w.chunk_cursor.p, 0, (size_t)P * sizeof(uint32_t), b->stream));
        launch_star_count(b->dp, max_pending, b->stream);
        launch_star_scan(b->dp, b->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(take.data(), w.nbr_take.p, (size_t)P * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipMemcpyAsync(total.data(), w.nbr_total.p, (size_t)P * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
        uint32_t max_take = 0, max_total = 0;
        for (uint32_t p = 0; p < P; ++p) {
            max_take = take[p] > max_take ? take[p] : max_take;
            max_total = total[p] > max_total ? total[p] : max_total;
        }
        if (max_take == 0) return fail(OXHIP_ERR_HIP, "RRT* wiring: no node fits the neighbour pool");   // (a list is at most cap <= pool_share long)
        // every pending node of every problem fits this round and the counting pass could keep all it found: the lists are
        // built from its chunks; otherwise (a pool segment or the chunk store ran out) the round searches a second time
        HIP_TRY(hipMemcpyAsync(chunks_used.data(), w.chunk_cursor.p, (size_t)P * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
        bool one_pass = (b->dp.dbg_flags & OXHIP_DEBUG_STAR_TWO_PASS) == 0;
        uint32_t max_chunks = 0;
        for (uint32_t p = 0; p < P; ++p) {
            const uint32_t pend = states[p].n_nodes > wired[p] ? states[p].n_nodes - wired[p] : 0u;
            if (take[p] != pend || chunks_used[p] > b->dp.chunk_share) one_pass = false;
            max_chunks = chunks_used[p] > max_chunks ? chunks_used[p] : max_chunks;
        }
        if (one_pass) launch_star_compact(b->dp, max_chunks, b->stream);
        else launch_star_fill(b->dp, max_take, b->stream);
        // The pairs are checked segment by segment (of the entries) and a segment's nodes -- those whose lists end inside it --
        // are wired on a second stream meanwhile: the wiring kernel is one latency-bound wave per problem and shares the
        // chip with the next segment's throughput-bound edge kernel at almost no cost to either
        const uint32_t segs = (max_total >= 64u * 1024u && (b->dp.dbg_flags & OXHIP_DEBUG_STAR_ONE_SEGMENT) == 0) ? 8u : 1u;
        for (uint32_t sgi = 0; sgi < segs; ++sgi) {
            b->dp.seg_index = sgi;
            b->dp.seg_count = segs;
            launch_star_edges(b->dp, max_total / segs + 2u, b->stream);
            HIP_TRY(hipEventRecord(w.ev_seg[sgi], b->stream));
            HIP_TRY(hipStreamWaitEvent(w.stream2, w.ev_seg[sgi], 0));
            launch_star_wire(b->dp, w.stream2);
        }
        HIP_TRY(hipEventRecord(w.ev_join, w.stream2));
        HIP_TRY(hipStreamWaitEvent(b->stream, w.ev_join, 0));
        HIP_TRY(hipGetLastError());
    }
}

// R^n's launch: by planner and by the kernel kind create() resolved (KERNEL_AUTO among them), for frozen and growing launches alike
static int32_t solve_real_vector(oxhip_rrt_batch* b) {
    const uint32_t kind = b->solve.kernel_kind;
    if (b->cfg.planner == OXHIP_PLANNER_RRT_CONNECT) launch_rrt_connect(b->dp, b->stream);
    else if (b->cfg.planner == OXHIP_PLANNER_RRT_STAR && b->star.wiring.on) {
        // geometry: exactly RRT's loop on the same stream (rrt_star_wire.hip's header); then wire the new nodes
        if (b->star.wiring.geo_cells) { launch_rrt_cells(b->dp, b->stream); b->dp.cells_meta_ok = 1; } else launch_rrt_lanes(b->dp, b->stream);
        HIP_TRY(hipGetLastError());
        OX_TRY(wire_new_nodes(b));
    }
    else if (b->cfg.planner == OXHIP_PLANNER_RRT_STAR) launch_rrt_star(b->dp, b->stream);
    else if (kind == OXHIP_KERNEL_CELLS) {
        launch_rrt_cells(b->dp, b->stream);
        b->dp.cells_meta_ok = 1;
        if (b->dp.freeze) { b->cells.board_last = (int32_t)b->dp.cells_parity; b->dp.cells_parity ^= 1u; }   // (the next frozen launch counts on the board this one cleared)
    }
    else if (kind == OXHIP_KERNEL_LANES) launch_rrt_lanes(b->dp, b->stream);
    else if (kind == OXHIP_KERNEL_RESIDENT) launch_rrt_resident(b->dp, b->stream);
    else launch_rrt_stream(b->dp, b->stream);
    return OXHIP_OK;
}

int32_t oxhip_rrt_batch_solve(oxhip_rrt_batch* b, uint64_t max_iterations, double timeout_s, uint32_t freeze,
                              int32_t* status_out) {
    if (!b) return fail(OXHIP_ERR_BAD_ARG, "null batch");
    drop_derived(b);
    OX_TRY(ready(b));
    if (b->cfg.planner != OXHIP_PLANNER_RRT && freeze) return fail(OXHIP_ERR_BAD_ARG, "freeze is for the RRT planner");
    if (space_of(b).midpoint_filter) OX_TRY(refresh_filter(b));
    if (std::isnan(timeout_s) || timeout_s < 0.0)   // Duration cannot be negative; from_secs_f32 (oxmpl-py rrt.rs:112) panics on both
        return fail(OXHIP_ERR_BAD_ARG, "timeout_s is NaN or negative (0 or +inf = no wall-clock limit)");
    const bool has_timeout = timeout_s > 0.0 && std::isfinite(timeout_s);
    const auto t0 = std::chrono::steady_clock::now();
    // The budget is always cut into bounded launches: the host reads the stop reasons in between, so a problem that can
    // never finish (start enclosed, huge budget) costs one chunk at a time instead of pinning the GPU for 2^40 iterations,
    // and with a timeout the host clock is consulted at the same points (rrt.rs:172-174).  Results do not depend on the
    // cut (a launch resumes from the state array).  A launch's budget stays below 2^31 (32-bit query counters).
    const uint64_t kChunk = has_timeout ? 2048 : 65536;
    const uint64_t chunk = max_iterations < kChunk ? max_iterations : kChunk;
    uint64_t remaining = max_iterations;
    Solve& sv = b->solve;
    sv.last_kernel_ms = 0.0;
    sv.last_launches = 0;
    bool timed_out = false;
    std::vector<ProblemState> states;
    while (remaining > 0) {
        uint64_t step = remaining < chunk ? remaining : chunk;
        b->dp.budget = step;
        b->dp.freeze = freeze ? 1 : 0;
        HIP_TRY(sv.clk.mark(Solve::kBegin, b->stream));
        OX_TRY(space_of(b).solve(b));
        HIP_TRY(hipGetLastError());
        HIP_TRY(sv.clk.mark(Solve::kEnd, b->stream));
        OX_TRY(read_states(b, states));   // (the launch's one synchronisation: the stop reasons come with it)
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, sv.clk.event(Solve::kBegin), sv.clk.event(Solve::kEnd)));
        sv.last_kernel_ms += ms;
        sv.last_launches++;
        remaining -= step;
        if (remaining == 0) break;
        bool any_running = false;
        for (auto& s : states) if (s.stop_reason == OXHIP_STOP_ITERATIONS) { any_running = true; break; }
        if (!any_running) break;
        if (has_timeout && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s) {
            timed_out = true;  // rrt.rs:172-174
            break;
        }
    }
    if (states.empty()) OX_TRY(read_states(b, states));   // (no launch: max_iterations = 0)
    for (auto& s : states)
        if (s.stop_reason == OXHIP_STOP_INTERNAL) return fail(OXHIP_ERR_HIP, "resident kernel: scanner/resolver hand-off stalled");
    if (timed_out) {
        for (auto& s : states) if (s.stop_reason == OXHIP_STOP_ITERATIONS) s.stop_reason = OXHIP_STOP_TIMEOUT;
        HIP_TRY(hipMemcpyAsync(b->trees.state.p, states.data(), states.size() * sizeof(ProblemState), hipMemcpyHostToDevice, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
    }
    if (status_out)
        for (uint32_t p = 0; p < b->cfg.n_problems; ++p) {
            const ProblemState& s = states[p];
            status_out[p] = s.goal_node >= 0 ? OXHIP_OK
                          : (s.stop_reason == OXHIP_STOP_TIMEOUT ? OXHIP_ERR_TIMEOUT : OXHIP_ERR_NO_SOLUTION_FOUND);
        }
    return OXHIP_OK;
}

int32_t oxhip_rrt_batch_get_counts(oxhip_rrt_batch* b, uint64_t* iterations, uint32_t* nodes, uint64_t* accepted,
                                   uint64_t* checksum, int32_t* goal_node, int32_t* stop_reason) {
    OX_TRY(ready(b));
    std::vector<ProblemState> states;
    OX_TRY(read_states(b, states));
    if (b->cfg.planner == OXHIP_PLANNER_RRT_STAR) {   // reported checksum = H (iterations) + W (wiring), DESIGN.md section 10
        std::vector<uint64_t> w(b->cfg.n_problems);
        HIP_TRY(hipMemcpyAsync(w.data(), b->star.wire_chk.p, w.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
        for (uint32_t p = 0; p < b->cfg.n_problems; ++p) states[p].checksum += w[p];
    }
    for (uint32_t p = 0; p < b->cfg.n_problems; ++p) {
        if (iterations) iterations[p] = states[p].iterations;
        if (nodes) nodes[p] = states[p].n_nodes;
        if (accepted) accepted[p] = states[p].accepted;
        if (checksum) checksum[p] = states[p].checksum;
        if (goal_node) goal_node[p] = states[p].goal_node;
        if (stop_reason) stop_reason[p] = states[p].stop_reason;
    }
    return OXHIP_OK;
}

static int32_t fetch_tree(oxhip_rrt_batch* b, uint32_t problem, uint32_t n, std::vector<double>& soa,
                          std::vector<int32_t>& parents, bool goal_tree = false) {
    const uint32_t dim = b->cfg.dim, cap = b->dp.cap;
    const double* tree_base = goal_tree ? b->trees.tree_b.p : b->trees.tree.p;
    const int32_t* parent_base = goal_tree ? b->trees.parent_b.p : b->trees.parent.p;
    soa.resize((size_t)dim * n);
    parents.resize(n);
    // [dim][n] out of [dim][cap]
    HIP_TRY(hipMemcpy2DAsync(soa.data(), (size_t)n * sizeof(double), tree_base + (size_t)problem * dim * cap,
                             (size_t)cap * sizeof(double), (size_t)n * sizeof(double), dim, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipMemcpyAsync(parents.data(), parent_base + (size_t)problem * cap, (size_t)n * sizeof(int32_t),
                           hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return OXHIP_OK;
}

// One problem's start tree or (RRTConnect) goal tree, as [n][dim] rows and parent indices.
static int32_t copy_tree(oxhip_rrt_batch* b, uint32_t problem, bool goal_tree, double* states_out, int32_t* parents_out,
                         uint32_t cap_nodes, uint32_t* n_nodes) {
    if (!b || !n_nodes) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    OX_TRY(setup_done(b));
    if (goal_tree && b->cfg.planner != OXHIP_PLANNER_RRT_CONNECT) return fail(OXHIP_ERR_BAD_ARG, "not an RRTConnect batch");
    OX_TRY(in_range(b, problem));
    OX_TRY(select_device(b->cfg.device));
    std::vector<ProblemState> states;
    OX_TRY(read_states(b, states));
    const uint32_t n = goal_tree ? states[problem].n_nodes_b : states[problem].n_nodes, dim = b->cfg.dim;
    *n_nodes = n;
    if (n > cap_nodes || (!states_out && !parents_out)) return n > cap_nodes ? fail(OXHIP_ERR_CAPACITY, "tree buffer too small") : OXHIP_OK;
    std::vector<double> soa;
    std::vector<int32_t> par;
    OX_TRY(fetch_tree(b, problem, n, soa, par, goal_tree));
    if (states_out)
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t k = 0; k < dim; ++k) states_out[(size_t)i * dim + k] = soa[(size_t)k * n + i];
    if (parents_out) std::memcpy(parents_out, par.data(), (size_t)n * sizeof(int32_t));
    return OXHIP_OK;
}

int32_t oxhip_rrt_batch_get_tree(oxhip_rrt_batch* b, uint32_t problem, double* states_out, int32_t* parents_out,
                                 uint32_t cap_nodes, uint32_t* n_nodes) {
    return copy_tree(b, problem, false, states_out, parents_out, cap_nodes, n_nodes);
}

int32_t oxhip_rrt_batch_get_path(oxhip_rrt_batch* b, uint32_t problem, double* states_out, uint32_t cap_states,
                                 uint32_t* len) {
    if (!b || !len) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    OX_TRY(ready(b, problem));
    std::vector<ProblemState> states;
    OX_TRY(read_states(b, states));
    *len = 0;
    const int32_t goal = states[problem].goal_node;
    if (goal < 0) return OXHIP_OK;
    const uint32_t n = states[problem].n_nodes, dim = b->cfg.dim;
    std::vector<double> soa;
    std::vector<int32_t> par;
    OX_TRY(fetch_tree(b, problem, n, soa, par));
    // reconstruct_path (rrt.rs:118-128): follow parents from the goal node, reverse
    std::vector<uint32_t> chain;
    for (int64_t i = goal; i >= 0; i = par[(size_t)i]) {
        chain.push_back((uint32_t)i);
        if (chain.size() > n) return fail(OXHIP_ERR_HIP, "parent chain is cyclic (corrupt tree)");
    }
    // RRTConnect (rrt_connect.rs:288-304): append the goal-tree chain from the connection node's parent to
    // the goal root (the reversed goal path with its first element, the duplicate connection point, skipped)
    std::vector<double> soa_b;
    std::vector<int32_t> par_b;
    std::vector<uint32_t> chain_b;
    const uint32_t nb = states[problem].n_nodes_b;
    if (b->cfg.planner == OXHIP_PLANNER_RRT_CONNECT && states[problem].goal_node_b >= 0) {
        OX_TRY(fetch_tree(b, problem, nb, soa_b, par_b, true));
        for (int64_t i = par_b[(size_t)states[problem].goal_node_b]; i >= 0; i = par_b[(size_t)i]) {
            chain_b.push_back((uint32_t)i);
            if (chain_b.size() > nb) return fail(OXHIP_ERR_HIP, "goal-tree parent chain is cyclic (corrupt tree)");
        }
    }
    const size_t total = chain.size() + chain_b.size();
    *len = (uint32_t)total;
    if (total > cap_states || !states_out) return total > cap_states ? fail(OXHIP_ERR_CAPACITY, "path buffer too small") : OXHIP_OK;
    for (size_t j = 0; j < chain.size(); ++j) {
        uint32_t i = chain[chain.size() - 1 - j];
        for (uint32_t k = 0; k < dim; ++k) states_out[j * dim + k] = soa[(size_t)k * n + i];
    }
    for (size_t j = 0; j < chain_b.size(); ++j)
        for (uint32_t k = 0; k < dim; ++k) states_out[(chain.size() + j) * dim + k] = soa_b[(size_t)k * nb + chain_b[j]];
    return OXHIP_OK;
}

int32_t oxhip_rrt_batch_get_goal_counts(oxhip_rrt_batch* b, uint32_t* nodes, int32_t* end_node) {
    OX_TRY(setup_done(b));
    if (b->cfg.planner != OXHIP_PLANNER_RRT_CONNECT) return fail(OXHIP_ERR_BAD_ARG, "not an RRTConnect batch");
    OX_TRY(select_device(b->cfg.device));
    std::vector<ProblemState> states;
    OX_TRY(read_states(b, states));
    for (uint32_t p = 0; p < b->cfg.n_problems; ++p) {
        if (nodes) nodes[p] = states[p].n_nodes_b;
        if (end_node) end_node[p] = states[p].goal_node_b;
    }
    return OXHIP_OK;
}

int32_t oxhip_rrt_batch_get_goal_tree(oxhip_rrt_batch* b, uint32_t problem, double* states_out, int32_t* parents_out,
                                      uint32_t cap_nodes, uint32_t* n_nodes) {
    return copy_tree(b, problem, true, states_out, parents_out, cap_nodes, n_nodes);
}

int32_t oxhip_rrt_batch_get_costs(oxhip_rrt_batch* b, uint32_t problem, double* costs, uint32_t cap_nodes, uint32_t* n_nodes) {
    if (!b || !n_nodes) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    OX_TRY(setup_done(b));
    if (b->cfg.planner != OXHIP_PLANNER_RRT_STAR) return fail(OXHIP_ERR_BAD_ARG, "not an RRT* batch");
    OX_TRY(in_range(b, problem));
    OX_TRY(select_device(b->cfg.device));
    std::vector<ProblemState> states;
    OX_TRY(read_states(b, states));
    const uint32_t n = states[problem].n_nodes;
    *n_nodes = n;
    if (!costs) return OXHIP_OK;
    if (n > cap_nodes) return fail(OXHIP_ERR_CAPACITY, "cost buffer too small");
    HIP_TRY(hipMemcpyAsync(costs, b->star.cost.p + (size_t)problem * b->dp.cap, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return OXHIP_OK;
}

// ------------------------------------------------------------------ the whole batch's paths (path_simplify.hip, shortcut_core.hip)

int32_t oxhip_rrt_batch_extract_paths(oxhip_rrt_batch* b) {
    OX_TRY(ready(b));
    Paths& ps = b->paths;
    ps.drop();
    const uint32_t P = b->cfg.n_problems, dim = b->cfg.dim;
    OX_TRY(clock_of(ps.clk, 3));
    PhaseClock& clk = *ps.clk;
    HIP_TRY(grow(ps.len, P));
    HIP_TRY(grow(ps.len_a, P));
    HIP_TRY(grow(ps.d_off, (size_t)P + 1));
    PathArgs a{ps.d_off.p, ps.len.p, ps.len_a.p, nullptr};
    // lengths first, one prefix sum, then the rows
    HIP_TRY(clk.mark(Paths::kBegin, b->stream));
    launch_path_len(b->dp, a, b->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(clk.mark(Paths::kMid, b->stream));
    ps.h_len.resize(P);
    HIP_TRY(hipMemcpyAsync(ps.h_len.data(), ps.len.p, (size_t)P * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, clk.event(Paths::kBegin), clk.event(Paths::kMid)));
    ps.ms[0] = ms;
    ps.off.assign((size_t)P + 1, 0);
    for (uint32_t p = 0; p < P; ++p) {
        if (ps.h_len[p] == 0xFFFFFFFFu) return fail(OXHIP_ERR_HIP, "parent chain is cyclic or leaves the tree (corrupt tree)");
        ps.off[p + 1] = ps.off[p] + ps.h_len[p];
    }
    const uint64_t total = ps.off[P];
    HIP_TRY(grow(ps.rows, (size_t)total * dim));
    HIP_TRY(hipMemcpyAsync(ps.d_off.p, ps.off.data(), ((size_t)P + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, b->stream));
    a.rows = ps.rows.p;
    HIP_TRY(clk.mark(Paths::kBegin, b->stream));
    launch_path_rows(b->dp, a, b->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(clk.mark(Paths::kMid, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipEventElapsedTime(&ms, clk.event(Paths::kBegin), clk.event(Paths::kMid)));
    ps.ms[0] += ms;
    ps.ok = true;
    return OXHIP_OK;
}

int32_t oxhip_rrt_batch_get_paths(oxhip_rrt_batch* b, uint64_t* offsets_out, double* states_out, uint64_t cap_states, uint64_t* total_out) {
    if (!b || !total_out) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    OX_TRY(setup_done(b));
    if (!b->paths.ok) return fail(OXHIP_ERR_BAD_ARG, "no extracted paths: call oxhip_rrt_batch_extract_paths after the last setup / solve / set_tree");
    OX_TRY(select_device(b->cfg.device));
    const uint32_t P = b->cfg.n_problems;
    const uint64_t total = b->paths.off[P];
    *total_out = total;
    if (offsets_out) std::memcpy(offsets_out, b->paths.off.data(), ((size_t)P + 1) * sizeof(uint64_t));
    if (total > cap_states) return fail(OXHIP_ERR_CAPACITY, "path buffer too small");
    if (!states_out || total == 0) return OXHIP_OK;
    HIP_TRY(hipMemcpyAsync(states_out, b->paths.rows.p, (size_t)total * b->cfg.dim * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return OXHIP_OK;
}

// the batch's parameters as the pair kernel reads them (R^n: the radii and the absolute margin of motion_seq.hpp's midpoint filter)
static int32_t pair_params(oxhip_rrt_batch* b, double& filt_base) {
    filt_base = 0.0;
    if (!space_of(b).midpoint_filter) return OXHIP_OK;
    if (b->obs.n_spheres != 0) OX_TRY(upload_radii(b));
    filt_base = 1e-9 * filter_maxabs(b->cfg, b->obs.sph_centres, nullptr);   // (no starts: the kernel widens it per motion)
    return OXHIP_OK;
}

static int32_t simplify_supported(const oxhip_rrt_batch* b) {
    if (space_of(b).no_simplify) return fail(OXHIP_ERR_BAD_ARG, space_of(b).no_simplify);
    if (b->cfg.dim < 2 && b->cfg.space == OXHIP_SPACE_REAL_VECTOR)   // (R^1; SO(2)'s one angle is built)
        return fail(OXHIP_ERR_BAD_ARG, "simplify_paths is not built for dim 1 (R^2 .. R^8 and SO(3))");
    return OXHIP_OK;
}

int32_t oxhip_rrt_batch_simplify_paths(oxhip_rrt_batch* b, uint32_t max_span, uint32_t chunk_problems) {
    OX_TRY(setup_done(b));
    OX_TRY(simplify_supported(b));
    OX_TRY(select_device(b->cfg.device));
    Paths& ps = b->paths;
    ps.simp_ok = false;
    if (!ps.ok) OX_TRY(oxhip_rrt_batch_extract_paths(b));
    const uint32_t P = b->cfg.n_problems;
    const uint64_t total = ps.off[P];
    double filt_base = 0.0;
    OX_TRY(pair_params(b, filt_base));
    HIP_TRY(grow(ps.sp_cost, total));
    HIP_TRY(grow(ps.sp_par, total));
    HIP_TRY(grow(ps.sp_idx, total));
    HIP_TRY(grow(ps.sp_len, P));
    HIP_TRY(grow(ps.sp_raw, P));
    HIP_TRY(grow(ps.sp_simp, P));
    HIP_TRY(grow(ps.sp_checks, P));
    std::vector<uint32_t> first;   // the rounds: as many problems each as the bit workspace (and the caller's override) allows
    uint32_t refused = 0;
    if (!shortcut_rounds(ps.h_len.data(), P, 1, max_span, kShortcutMatrixBytes, chunk_problems, first, refused))
        return fail(OXHIP_ERR_CAPACITY, "a path's pair matrix exceeds the 1 GiB workspace: pass a max_span");
    OX_TRY(clock_of(ps.clk, 3));
    PhaseClock& clk = *ps.clk;
    ps.ms[1] = ps.ms[2] = 0.0;
    ps.rounds = 0;
    std::vector<uint64_t> woff;
    for (size_t r = 0; r + 1 < first.size(); ++r) {
        const uint32_t q0 = first[r], n_chunk = first[r + 1] - q0;
        woff.assign(1, 0);
        for (uint32_t q = q0; q < q0 + n_chunk; ++q) woff.push_back(woff.back() + shortcut_shape(ps.h_len[q], 1, max_span).words);
        HIP_TRY(grow(ps.sp_woff, (size_t)n_chunk + 1));
        HIP_TRY(grow(ps.sp_bits, woff.back()));
        HIP_TRY(hipMemcpyAsync(ps.sp_woff.p, woff.data(), woff.size() * sizeof(uint64_t), hipMemcpyHostToDevice, b->stream));
        // the extracted rows are the shortcut's rows (m = 1); the per-problem tables from q0 on, the per-row ones whole
        const ShortcutArgs a{ps.len.p + q0, ps.d_off.p + q0, ps.rows.p, ps.sp_woff.p, ps.sp_bits.p, woff.back(), n_chunk, 1, max_span, 0, filt_base};
        const ShortcutOut out{ps.sp_cost.p, ps.sp_par.p, ps.sp_idx.p, ps.sp_len.p + q0, ps.sp_raw.p + q0, ps.sp_simp.p + q0, ps.sp_checks.p + q0};
        HIP_TRY(clk.mark(Paths::kBegin, b->stream));
        launch_shortcut_pairs(b->dp, a, false, b->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(clk.mark(Paths::kMid, b->stream));
        launch_shortcut_dp(b->dp.space, b->dp.dim, a, out, b->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(clk.mark(Paths::kEnd, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));   // (woff is rebuilt by the next round)
        ps.ms[1] += clk.ms(Paths::kBegin, Paths::kMid);
        ps.ms[2] += clk.ms(Paths::kMid, Paths::kEnd);
        ps.rounds++;
    }
    ps.simp_ok = true;
    return OXHIP_OK;
}

int32_t oxhip_rrt_batch_get_simplified_paths(oxhip_rrt_batch* b, uint64_t* offsets_out, double* states_out, uint32_t* indices_out,
                                             uint64_t cap_states, uint64_t* total_out) {
    if (!b || !total_out) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    OX_TRY(setup_done(b));
    if (!b->paths.simp_ok || !b->paths.ok)
        return fail(OXHIP_ERR_BAD_ARG, "no simplified paths: call oxhip_rrt_batch_simplify_paths after the last setup / solve / set_tree");
    OX_TRY(select_device(b->cfg.device));
    const uint32_t P = b->cfg.n_problems, dim = b->cfg.dim;
    std::vector<uint32_t> slen(P);
    HIP_TRY(hipMemcpyAsync(slen.data(), b->paths.sp_len.p, (size_t)P * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    std::vector<uint64_t> soff((size_t)P + 1, 0);
    for (uint32_t p = 0; p < P; ++p) soff[p + 1] = soff[p] + slen[p];
    const uint64_t total = soff[P];
    *total_out = total;
    if (offsets_out) std::memcpy(offsets_out, soff.data(), soff.size() * sizeof(uint64_t));
    if (total > cap_states) return fail(OXHIP_ERR_CAPACITY, "path buffer too small");
    if ((!states_out && !indices_out) || total == 0) return OXHIP_OK;
    // one copy of the raw rows and of the index lists; the simplified rows are gathered from them
    const std::vector<uint64_t>& off = b->paths.off;
    const uint64_t raw_total = off[P];
    std::vector<uint32_t> idx(raw_total);
    std::vector<double> rows;
    HIP_TRY(hipMemcpyAsync(idx.data(), b->paths.sp_idx.p, (size_t)raw_total * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream));
    if (states_out) {
        rows.resize((size_t)raw_total * dim);
        HIP_TRY(hipMemcpyAsync(rows.data(), b->paths.rows.p, rows.size() * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    }
    HIP_TRY(hipStreamSynchronize(b->stream));
    for (uint32_t p = 0; p < P; ++p)
        for (uint32_t t = 0; t < slen[p]; ++t) {
            const uint32_t i = idx[off[p] + t];
            if (indices_out) indices_out[soff[p] + t] = i;
            if (states_out) std::memcpy(states_out + (soff[p] + t) * dim, rows.data() + (off[p] + i) * dim, dim * sizeof(double));
        }
    return OXHIP_OK;
}

int32_t oxhip_rrt_batch_get_simplify_results(oxhip_rrt_batch* b, double* raw_cost, double* simplified_cost, uint64_t* checks) {
    OX_TRY(setup_done(b));
    if (!b->paths.simp_ok || !b->paths.ok)
        return fail(OXHIP_ERR_BAD_ARG, "no simplified paths: call oxhip_rrt_batch_simplify_paths after the last setup / solve / set_tree");
    OX_TRY(select_device(b->cfg.device));
    const size_t P = b->cfg.n_problems;
    if (raw_cost) HIP_TRY(hipMemcpyAsync(raw_cost, b->paths.sp_raw.p, P * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    if (simplified_cost) HIP_TRY(hipMemcpyAsync(simplified_cost, b->paths.sp_simp.p, P * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    if (checks) HIP_TRY(hipMemcpyAsync(checks, b->paths.sp_checks.p, P * sizeof(uint64_t), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return OXHIP_OK;
}

int32_t oxhip_rrt_batch_path_valid_matrix(oxhip_rrt_batch* b, uint32_t problem, uint32_t max_span, uint8_t* out, uint64_t cap_bytes,
                                          uint32_t* len_out) {
    if (!b || !len_out) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    OX_TRY(setup_done(b, problem));
    OX_TRY(simplify_supported(b));
    if (!b->paths.ok) return fail(OXHIP_ERR_BAD_ARG, "no extracted paths: call oxhip_rrt_batch_extract_paths after the last setup / solve / set_tree");
    OX_TRY(select_device(b->cfg.device));
    const uint32_t L = b->paths.h_len[problem];
    *len_out = L;
    if ((uint64_t)L * L > cap_bytes) return fail(OXHIP_ERR_CAPACITY, "matrix buffer too small");
    if (!out || L == 0) return OXHIP_OK;
    const ShortcutShape sh = shortcut_shape(L, 1, max_span);
    const uint64_t words = sh.words;
    if (!shortcut_fits(sh, kShortcutMatrixBytes)) return fail(OXHIP_ERR_CAPACITY, "a path's pair matrix exceeds the 1 GiB workspace: pass a max_span");
    double filt_base = 0.0;
    OX_TRY(pair_params(b, filt_base));
    // the pair kernel on a round of this one problem (its own buffers: a simplified result stays as it is)
    DevBuf<uint64_t> d_woff, d_bits;
    const uint64_t woff[2] = {0, words};
    OX_TRY(to_device(d_woff, woff, 2, b->stream));
    HIP_TRY(d_bits.alloc(words ? words : 1));
    const ShortcutArgs a{b->paths.len.p + problem, b->paths.d_off.p + problem, b->paths.rows.p, d_woff.p, d_bits.p, words, 1, 1, max_span, 0, filt_base};
    launch_shortcut_pairs(b->dp, a, false, b->stream);
    HIP_TRY(hipGetLastError());
    std::vector<uint64_t> bits(words);
    OX_TRY(to_host(bits.data(), d_bits, words, b->stream));
    shortcut_matrix_bytes(bits.data(), L, 1, max_span, out);
    return OXHIP_OK;
}

int32_t oxhip_rrt_batch_paths_last_timing(oxhip_rrt_batch* b, double* extract_ms, double* pairs_ms, double* dp_ms, uint32_t* rounds) {
    if (!b) return fail(OXHIP_ERR_BAD_ARG, "null batch");
    if (extract_ms) *extract_ms = b->paths.ms[0];
    if (pairs_ms) *pairs_ms = b->paths.ms[1];
    if (dp_ms) *dp_ms = b->paths.ms[2];
    if (rounds) *rounds = b->paths.rounds;
    return OXHIP_OK;
}

int32_t oxhip_rrt_batch_last_timing(oxhip_rrt_batch* b, double* kernel_ms, uint32_t* launches, uint32_t* kernel_kind) {
    if (!b) return fail(OXHIP_ERR_BAD_ARG, "null batch");
    if (kernel_ms) *kernel_ms = b->solve.last_kernel_ms;
    if (launches) *launches = b->solve.last_launches;
    if (kernel_kind) *kernel_kind = b->solve.kernel_kind;
    return OXHIP_OK;
}

int32_t oxhip_rrt_batch_enable_stamps(oxhip_rrt_batch* b, uint32_t enable) {
    if (!b) return fail(OXHIP_ERR_BAD_ARG, "null batch");
    OX_TRY(select_device(b->cfg.device));
    if (enable) {
        HIP_TRY(b->dbg.alloc(OXHIP_STAMP_WORDS));
        HIP_TRY(hipMemsetAsync(b->dbg.p, 0, OXHIP_STAMP_WORDS * sizeof(uint64_t), b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
        b->dp.dbg = b->dbg.p;
    } else {
        b->dp.dbg = nullptr;
    }
    return OXHIP_OK;
}

int32_t oxhip_rrt_batch_get_stamps(oxhip_rrt_batch* b, uint64_t* out, uint32_t cap_words) {
    if (!b || !out) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    if (!b->dp.dbg) return fail(OXHIP_ERR_BAD_ARG, "stamps are not enabled");
    OX_TRY(select_device(b->cfg.device));
    const uint32_t n = cap_words < OXHIP_STAMP_WORDS ? cap_words : OXHIP_STAMP_WORDS;
    if (n) HIP_TRY(hipMemcpyAsync(out, b->dbg.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (n > OXHIP_STAMP_CELLS_BOARD && b->dp.cell_board && b->cells.board_last >= 0) {
        // rrt_cells.hip: what the last frozen launch's progress board holds, summed over the XCDs
        std::vector<uint64_t> board(kCellsBoardWords);
        HIP_TRY(hipMemcpy(board.data(), b->dp.cell_board + (size_t)b->cells.board_last * kCellsBoardWords, kCellsBoardWords * sizeof(uint64_t), hipMemcpyDeviceToHost));
        uint64_t sum = 0;
        for (uint32_t x = 0; x < 8; ++x) sum += board[x * (kCellsBoardWords / 8)];
        out[OXHIP_STAMP_CELLS_BOARD] = sum;
    }
    return OXHIP_OK;
}

// ------------------------------------------------------------------ stand-alone primitives

int32_t oxhip_nn_argmin_batch(int32_t device, uint32_t dim, const double* nodes, const uint32_t* n_nodes,
                              uint32_t n_queries, const double* queries, uint32_t* out_index, double* out_min_dist) {
    if (!nodes || !n_nodes || !queries || !out_index || !out_min_dist) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    if (dim == 0 || dim > OXHIP_MAX_DIM) return fail(OXHIP_ERR_BAD_ARG, "dim must be in 1..8");
    if (n_queries == 0) return OXHIP_OK;
    OX_TRY(select_device(device));
    std::vector<uint64_t> offsets(n_queries);
    uint64_t total = 0;
    for (uint32_t q = 0; q < n_queries; ++q) {
        if (n_nodes[q] == 0) return fail(OXHIP_ERR_BAD_ARG, "every tree needs at least its root (rrt.rs:188 reads tree[0])");
        offsets[q] = total;
        total += n_nodes[q];
    }
    PooledStream ts;
    OX_TRY(ts.acquire(device));
    DevBuf<double> d_nodes, d_q, d_dist;
    DevBuf<uint64_t> d_off;
    DevBuf<uint32_t> d_n, d_idx;
    OX_TRY(to_device(d_nodes, nodes, (size_t)total * dim, ts.s));
    OX_TRY(to_device(d_q, queries, (size_t)n_queries * dim, ts.s));
    OX_TRY(to_device(d_off, offsets.data(), n_queries, ts.s));
    OX_TRY(to_device(d_n, n_nodes, n_queries, ts.s));
    HIP_TRY(d_idx.alloc(n_queries));
    HIP_TRY(d_dist.alloc(n_queries));
    launch_nn_argmin(dim, d_nodes.p, d_off.p, d_n.p, n_queries, d_q.p, d_idx.p, d_dist.p, ts.s);
    HIP_TRY(hipGetLastError());
    OX_TRY(to_host(out_index, d_idx, n_queries, ts.s));
    OX_TRY(to_host(out_min_dist, d_dist, n_queries, ts.s));
    return OXHIP_OK;
}

int32_t oxhip_distance_batch(int32_t device, uint32_t dim, const double* a, const double* b, uint32_t n, double* out) {
    if (!a || !b || !out) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    if (dim == 0 || dim > OXHIP_MAX_DIM) return fail(OXHIP_ERR_BAD_ARG, "dim must be in 1..8");
    return op_batch(device, a, b, nullptr, n, out, dim, dim, 1, true, false,
                    [=](const double* da, const double* db, const double*, double* dout, hipStream_t s) { launch_distance(dim, da, db, n, dout, s); });
}

int32_t oxhip_interpolate_batch(int32_t device, uint32_t dim, const double* from, const double* to, const double* t,
                                uint32_t n, double* out) {
    if (!from || !to || !t || !out) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    if (dim == 0 || dim > OXHIP_MAX_DIM) return fail(OXHIP_ERR_BAD_ARG, "dim must be in 1..8");
    return op_batch(device, from, to, t, n, out, dim, dim, dim, true, true,
                    [=](const double* da, const double* db, const double* dt, double* dout, hipStream_t s) { launch_interpolate(dim, da, db, dt, n, dout, s); });
}

// ------------------------------------------------------------------ re-checking the trees (rrt_revalidate.hip)
int32_t oxhip_rrt_batch_revalidate_trees(oxhip_rrt_batch* b, uint32_t* n_removed, uint8_t* goal_lost) {
    if (!b) return fail(OXHIP_ERR_BAD_ARG, "null batch");
    OX_TRY(setup_done(b));
    if (b->cfg.planner == OXHIP_PLANNER_RRT_CONNECT)
        return fail(OXHIP_ERR_BAD_ARG, "revalidate_trees is for the RRT planner (an RRTConnect batch keeps two trees and their connection)");
    if (b->cfg.planner != OXHIP_PLANNER_RRT)
        return fail(OXHIP_ERR_BAD_ARG, "revalidate_trees is for the RRT planner (an RRT* batch would need its costs and wiring cursors pruned as well)");
    // below the refusals: a call refused for its planner leaves the batch's extracted and simplified paths as they were
    drop_derived(b);   // (the last call's map with them)
    OX_TRY(select_device(b->cfg.device));
    if (space_of(b).midpoint_filter) OX_TRY(refresh_filter(b));   // as solve does: the next launch reads them
    const uint32_t P = b->cfg.n_problems, cap = b->dp.cap;
    const bool so3 = b->cfg.space == OXHIP_SPACE_SO3;
    RevalArgs a{};
    OX_TRY(pair_params(b, a.filt_base));   // (R^n: the radii and the absolute margin of motion_seq.hpp's midpoint filter)
    std::vector<ProblemState> states;
    OX_TRY(read_states(b, states));        // one read of the state array: the node counts
    Reval& rv = b->reval;
    rv.n_before.resize(P);
    uint32_t max_n = 1;
    for (uint32_t p = 0; p < P; ++p) {
        rv.n_before[p] = states[p].n_nodes;
        if (states[p].n_nodes == 0 || states[p].n_nodes > cap) return fail(OXHIP_ERR_HIP, "revalidate_trees: a tree size outside 1..capacity");
        max_n = std::max(max_n, states[p].n_nodes);
    }
    a.tiles = (max_n + 255u) / 256u;
    if ((uint64_t)P * a.tiles * 256u > 0x7FFFFFFFull) return fail(OXHIP_ERR_CAPACITY, "revalidate_trees: more than 2^31 node slots");
    const size_t slots = (size_t)P * cap;
    HIP_TRY(grow(rv.edge_ok, slots));
    HIP_TRY(grow(rv.alive, slots));
    HIP_TRY(grow(rv.new_index, slots));
    HIP_TRY(grow(rv.jump, slots));
    HIP_TRY(grow(rv.n_after, P));
    HIP_TRY(grow(rv.n_removed, P));
    HIP_TRY(grow(rv.goal_lost, P));
    if (so3) {
        // 65 bytes per staged edge (two rows and a verdict) out of 6 bytes per slot: with the 10 above, 16 bytes per slot
        // (one block of 64 edges at the least)
        const size_t edges = std::max<size_t>(64, std::min<size_t>(slots * 6 / 65, (size_t)P * a.tiles * 256u));
        HIP_TRY(grow(rv.stage, edges * 65));
        a.stage_cap = (uint32_t)std::min<size_t>(edges, 0x7FFFFF00u);
        a.stage_from = reinterpret_cast<double*>(rv.stage.p);
        a.stage_to = a.stage_from + (size_t)a.stage_cap * 4;
        a.stage_out = reinterpret_cast<uint8_t*>(a.stage_to + (size_t)a.stage_cap * 4);
    }
    a.tree = b->trees.tree.p; a.parent = b->trees.parent.p; a.skip = b->trees.skip.p; a.state = b->trees.state.p;
    a.goal_c = b->goals.goal_c.p; a.goal_thr = b->goals.goal_thr.p;
    a.edge_ok = rv.edge_ok.p; a.alive = rv.alive.p; a.new_index = rv.new_index.p; a.jump = rv.jump.p;
    a.n_after = rv.n_after.p; a.n_removed = rv.n_removed.p; a.goal_lost = rv.goal_lost.p;
    a.cap = cap;
    OX_TRY(clock_of(rv.clk, 5));
    PhaseClock& clk = *rv.clk;
    HIP_TRY(clk.mark(Reval::kBegin, b->stream));
    launch_rrt_reval_edges(b->dp, a, P, b->stream);
    HIP_TRY(clk.mark(Reval::kEdgesEnd, b->stream));
    launch_rrt_reval_survive(a, P, b->stream);
    HIP_TRY(clk.mark(Reval::kSurviveEnd, b->stream));
    launch_rrt_reval_scan(a, P, b->stream);
    HIP_TRY(clk.mark(Reval::kScanEnd, b->stream));
    launch_rrt_reval_compact(b->dp, a, P, b->stream);
    HIP_TRY(clk.mark(Reval::kCompactEnd, b->stream));
    HIP_TRY(hipGetLastError());
    OX_TRY(reset_tree_caches(b, 0, P));   // (the trees were compacted in place)
    if (n_removed) HIP_TRY(hipMemcpyAsync(n_removed, rv.n_removed.p, (size_t)P * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream));
    if (goal_lost) HIP_TRY(hipMemcpyAsync(goal_lost, rv.goal_lost.p, P, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    for (int i = Reval::kBegin; i < Reval::kCompactEnd; ++i) rv.ms[i] = clk.ms(i, i + 1);
    rv.ok = true;
    return OXHIP_OK;
}

int32_t oxhip_rrt_batch_get_revalidate_map(oxhip_rrt_batch* b, uint32_t problem, int32_t* new_index, uint8_t* edge_ok, uint32_t cap,
                                           uint32_t* n_before) {
    if (!b || !n_before) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    OX_TRY(setup_done(b, problem));
    if (!b->reval.ok)
        return fail(OXHIP_ERR_BAD_ARG, "no revalidation map: call oxhip_rrt_batch_revalidate_trees after the last setup / solve / set_tree");
    OX_TRY(select_device(b->cfg.device));
    const uint32_t n = b->reval.n_before[problem];
    *n_before = n;
    if (cap < n) return fail(OXHIP_ERR_CAPACITY, "map buffer too small");
    const size_t base = (size_t)problem * b->dp.cap;
    if (new_index) HIP_TRY(hipMemcpyAsync(new_index, b->reval.new_index.p + base, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, b->stream));
    if (edge_ok) HIP_TRY(hipMemcpyAsync(edge_ok, b->reval.edge_ok.p + base, n, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return OXHIP_OK;
}

int32_t oxhip_rrt_batch_revalidate_last_timing(oxhip_rrt_batch* b, double* phase_ms) {
    if (!b || !phase_ms) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    for (int i = 0; i < 4; ++i) phase_ms[i] = b->reval.ms[i];
    return OXHIP_OK;
}

int32_t oxhip_rrt_batch_is_valid(oxhip_rrt_batch* b, const double* states, uint32_t n, uint8_t* out) {
    if (!b || !states || !out) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    if (n == 0) return OXHIP_OK;
    OX_TRY(select_device(b->cfg.device));
    DevBuf<double> ds;
    DevBuf<uint8_t> dout;
    OX_TRY(to_device(ds, states, (size_t)n * b->cfg.dim, b->stream));
    HIP_TRY(dout.alloc(n));
    space_of(b).is_valid(b, ds.p, n, dout.p);
    HIP_TRY(hipGetLastError());
    return to_host(out, dout, n, b->stream);
}

int32_t oxhip_rrt_batch_check_motion(oxhip_rrt_batch* b, const double* from, const double* to, uint32_t n, uint8_t* out) {
    if (!b || !from || !to || !out) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    if (n == 0) return OXHIP_OK;
    OX_TRY(select_device(b->cfg.device));
    DevBuf<double> da, db;
    DevBuf<uint8_t> dout;
    OX_TRY(to_device(da, from, (size_t)n * b->cfg.dim, b->stream));
    OX_TRY(to_device(db, to, (size_t)n * b->cfg.dim, b->stream));
    HIP_TRY(dout.alloc(n));
    space_of(b).check_motion(b, da.p, db.p, n, dout.p);
    HIP_TRY(hipGetLastError());
    return to_host(out, dout, n, b->stream);
}

int32_t oxhip_f64_op_batch(int32_t device, uint32_t op, const double* a, const double* b, const double* c, uint32_t n,
                           double* out) {
    if (!a || !out || op > 6) return fail(OXHIP_ERR_BAD_ARG, "bad argument");
    if ((op == 1 || op == 3 || op == 4) && !b) return fail(OXHIP_ERR_BAD_ARG, "operand b required");
    if (op == 3 && !c) return fail(OXHIP_ERR_BAD_ARG, "operand c required");
    return op_batch(device, a, b, c, n, out, 1, 1, 1, b != nullptr, c != nullptr,
                    [=](const double* da, const double* db, const double* dt, double* dout, hipStream_t s) { launch_f64_op(op, da, db, dt, n, dout, s); });
}

int32_t oxhip_se2_op_batch(int32_t device, uint32_t op, const double* a, const double* b, const double* t, uint32_t n,
                           double* out) {
    if (!a || !b || !out || op > 1 || (op == 1 && !t)) return fail(OXHIP_ERR_BAD_ARG, "bad argument");
    return op_batch(device, a, b, t, n, out, 3, 3, 3, true, t != nullptr,
                    [=](const double* da, const double* db, const double* dt, double* dout, hipStream_t s) { launch_se2_op(op, da, db, dt, n, dout, s); });
}

int32_t oxhip_so3_op_batch(int32_t device, uint32_t op, const double* a, const double* b, const double* t, uint32_t n,
                           double* out) {
    if (!a || !out || op > 2 || (op <= 1 && !b) || (op == 1 && !t)) return fail(OXHIP_ERR_BAD_ARG, "bad argument");
    return op_batch(device, a, b, t, n, out, op == 2 ? 1 : 4, 4, op == 1 ? 4 : 1, op <= 1, op == 1,
                    [=](const double* da, const double* db, const double* dt, double* dout, hipStream_t s) { launch_so3_op(op, da, db, dt, n, dout, s); });
}

int32_t oxhip_se3_op_batch(int32_t device, uint32_t op, const double* a, const double* b, const double* t, uint32_t n,
                           double* out) {
    if (!a || !b || !out || op > 2 || (op == 1 && !t)) return fail(OXHIP_ERR_BAD_ARG, "bad argument");
    return op_batch(device, a, b, t, n, out, 7, 7, op == 0 ? 1 : (op == 1 ? 7 : 3), true, op == 1,
                    [=](const double* da, const double* db, const double* dt, double* dout, hipStream_t s) { launch_se3_op(op, da, db, dt, n, dout, s); });
}

int32_t oxhip_rng_u64_batch(int32_t device, uint64_t seed, uint64_t stream, uint32_t n, uint64_t* out) {
    if (!out) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    if (n == 0) return OXHIP_OK;
    OX_TRY(select_device(device));
    PooledStream ts;
    OX_TRY(ts.acquire(device));
    DevBuf<uint64_t> dout;
    HIP_TRY(dout.alloc(n));
    launch_rng_u64(seed, stream, n, dout.p, ts.s);
    HIP_TRY(hipGetLastError());
    return to_host(out, dout, n, ts.s);
}

}  // extern "C"
