// oxhip_prm_api.hip -- the PRM part of the C ABI (include/oxmpl_hip.h, oxhip_prm_*).
//
// Host side of oxmpl's PRM (oxmpl/src/geometric/planners/prm.rs): owns the device roadmap and drives the kernels of prm_kernels.hip
// (space = OXHIP_SPACE_SO3: prm_so3.hip).  No CPU fallback: without a HIP device every computing entry point fails.
// Each entry point is a sequence of named steps ("PRM host side"): create = validate_prm_config, select_device,
// fill_prm_params, alloc_prm; construct_roadmap = the reference's loop over sample_until, knn_row_radii, find_pairs, knn_select,
// reserve_keys, check_edges, then build_csr; solve = query_sets, prm_bfs_path (oxhip_host.hpp, on the CSR roadmap copied back once per
// construction), the path; solve_batch[_shortest] (DESIGN.md sections 17, 19) = stage_batch, reserve_batch_workspace, then per round
// run_round, scatter_round, extract_round_paths; grow_roadmap = liveness_mask, grow_capacity, keys_from_csr,
// then grow_round: construction's steps for the new milestones, with drop_dead_candidates before the edges; components (DESIGN.md
// section 24) = components_of, then the copies; prune = prune_stage1_mask, components_of(alive), prune_stage2_mask, compact_roadmap.
// The space is named by the dispatchers below the handle, the per-space part of
// the sampler, the steps of create, the two obstacle setters and the prm_shortest launches that take it as an argument.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <deque>

#include "oxhip_host.hpp"
#include "oxhip_internal.hpp"
#include "rrt_device.hpp"

using namespace oxhip;

struct oxhip_prm {
    oxhip_prm_config cfg{};
    DevParams dp{};           // space, resolution and validity field (the RRT fields stay zero)
    PrmArgs args{};
    double thr_conn = -1.0;   // d2 <= thr_conn  <=>  distance < connection_radius
    bool so3 = false;         // OXHIP_SPACE_SO3: quaternion milestones, cones, prm_so3.hip
    double so3_lo = -1.0, so3_hi = -1.0;   // |dot| bands of the SO(3) radius test (so3_radius_bands)
    hipStream_t stream = nullptr;
    hipEvent_t ev[6] = {};
    DevBuf<double> ms, sph_c, sph_thr, sph_r, box_lo, box_hi;
    DevBuf<float> ms32;   // fl32 shadow of the milestones (pair-search screen)
    double maxabs = 1.0;      // largest |coordinate| of bounds and sphere centres (midpoint filter margin)
    DevBuf<PrmState> state;
    DevBuf<uint2> cand;
    // k-nearest variant: per-row candidate radii, the sorted candidates and their distances, the selected pairs
    DevBuf<double> knn_thr, knn_dist;
    DevBuf<float> knn_thr32;
    DevBuf<uint64_t> knn_keys, knn_sorted;
    DevBuf<uint2> knn_sel;
    DevBuf<uint32_t> knn_counters, knn_failed;
    uint32_t knn_failed_rows = 0;   // rows of the last construct_roadmap that needed the exact search
    DevBuf<uint64_t> keys, keys_sorted;
    DevBuf<uint8_t> sort_tmp;
    uint32_t n_keys = 0;       // directed edge entries of the constructed roadmap
    bool host_copy = false;    // h_offsets / h_nbrs / h_states are current
    DevBuf<uint32_t> offsets, nbrs, start_valid;
    DevBuf<uint8_t> flags;
    // parallel sampler scratch (one round)
    DevBuf<double> spec_tmp;
    DevBuf<uint64_t> spec_vbits;
    DevBuf<uint32_t> spec_off, spec_flag;
    DevBuf<uint64_t> spec_abits;   // SO(3) sampler: accepted-attempt ballots and counts
    DevBuf<uint32_t> spec_acnt;
    double valid_rate = 1.0;   // running estimate of P(sample is valid), sizes the rounds
    bool is_setup = false;
    PrmQuery query{};
    // host copy of the constructed roadmap
    uint32_t n = 0;
    uint64_t n_samples = 0;
    uint32_t redraw_batches = 0;
    std::vector<uint32_t> h_offsets, h_nbrs;
    std::vector<double> h_states;  // AoS [n][dim]
    // last query
    std::vector<uint32_t> start_conn, goal_idx;
    // phase timings of the last construct / solve (ms): sample, pairs, edges, sort+csr, query kernel, bfs (host)
    double t_ms[6] = {};
    uint64_t n_candidates = 0;
    // last oxhip_prm_solve_batch: its queries, per-query results and all paths; per-round device workspace
    bool batch_valid = false;
    uint32_t batch_rounds = 0;
    double batch_ms[4] = {};   // flag kernels, search kernels, path extraction, device-to-host copies
    std::vector<double> b_starts, b_goals, b_thr, b_filt;       // as uploaded: [Q][dim], [Q][dim], [Q], [Q]
    std::vector<int32_t> b_status, b_goal_node;
    std::vector<uint32_t> b_len, b_nstart, b_ngoal, b_nodes;
    std::vector<uint64_t> b_off;                                // [Q + 1] row offsets of the paths
    std::vector<double> b_rows;
    DevBuf<double> bd_starts, bd_goals, bd_thr, bd_filt, bd_rows;
    DevBuf<uint8_t> bd_flags;
    DevBuf<uint32_t> bd_start_valid, bd_parent, bd_queue, bd_res, bd_nodes;
    DevBuf<uint64_t> bd_off;
    hipEvent_t bev[7] = {};
    // oxhip_prm_solve_batch_shortest: the edge weights live until the roadmap changes; the rest is the last batch's
    int32_t batch_mode = -1;   // weights mode of the last batch, -1: it was the breadth-first oxhip_prm_solve_batch
    bool w_valid = false;      // w_edges holds the distances of the roadmap's CSR entries
    DevBuf<double> w_edges;
    double short_ms[6] = {};   // edge weights (when this batch computed them), flags + initial labels, label rounds, tight levels, paths, copies
    std::vector<double> b_cost;
    std::vector<uint32_t> b_rounds;
    std::vector<uint64_t> b_relaxed;
    DevBuf<uint64_t> bd_label;
    DevBuf<uint32_t> bd_stamp, bd_rounds;
    DevBuf<double> bd_cost;
    DevBuf<unsigned long long> bd_relaxed;
    hipEvent_t sev[2] = {};
    // oxhip_prm_revalidate: its workspace and the phase times of the last call
    DevBuf<uint8_t> rv_valid, rv_keep, rv_tmp;
    DevBuf<uint32_t> rv_pos, rv_nbrs, rv_counters;
    DevBuf<uint4> rv_pairs;
    DevBuf<uint2> rv_cand;       // SO(3): the pairs as construction's edge kernel reads them, the keys it emits and their count
    DevBuf<uint64_t> rv_keys;
    DevBuf<PrmState> rv_state;
    double reval_ms[4] = {};   // milestone validity, pair emission, edge checks, compaction
    // oxhip_prm_grow_roadmap: where the sampler stopped (stream id, u64 word), the filtered candidates, the
    // phase times of the last call
    bool pos_valid = false;    // set by construct_roadmap / grow_roadmap, forgotten by setup / set_roadmap
    uint64_t pos_stream = 0, pos_draws = 0;
    DevBuf<uint2> gw_cand;
    DevBuf<uint32_t> gw_count;
    double grow_ms[6] = {};    // liveness mask, keys from CSR, sample, pairs (+ filter), edges, sort + CSR
    // oxhip_prm_components / oxhip_prm_prune: the union-find's arrays (the labels, sizes and summary are
    // kept until the roadmap changes), the prune's masks, scans and second buffers, the phase times of the last calls
    bool cc_valid = false;     // cc_label / cc_size / cc_summary describe the roadmap as it stands
    DevBuf<uint32_t> cc_parent, cc_label, cc_count, cc_size;
    DevBuf<unsigned long long> cc_summary;
    DevBuf<uint8_t> pr_keep, pr_mask, pr_ekeep;
    DevBuf<uint32_t> pr_pos, pr_epos, pr_kept, pr_offsets, pr_nbrs;
    DevBuf<int32_t> pr_index;
    DevBuf<double> pr_ms;
    DevBuf<float> pr_ms32;
    hipEvent_t cev[10] = {};
    double cc_ms[4] = {};      // init + hook, flatten, sizes + summary, copies
    double prune_ms[5] = {};   // masks, components, scans, move entries, move states
};

namespace {

int32_t read_state(oxhip_prm* h, PrmState& st) {
    HIP_TRY(hipMemcpyAsync(&st, h->state.p, sizeof(PrmState), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return OXHIP_OK;
}

int32_t write_state(oxhip_prm* h, const PrmState& st) {
    HIP_TRY(hipMemcpyAsync(h->state.p, &st, sizeof(PrmState), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return OXHIP_OK;
}

// ---- the one place that names the space: which launcher, and whether a radius travels as given or as its squared threshold
void launch_pairs(oxhip_prm* h, uint32_t j0, uint32_t j1) {   // the k-nearest variant searches its per-row radii (knn_row_radii)
    if (h->so3) launch_prm_so3_pairs(h->args, j0, j1, h->so3_lo, h->so3_hi, h->cfg.connection_radius, h->stream);
    else if (h->cfg.knn_k) launch_prm_pairs(h->dp, h->args, j0, j1, std::numeric_limits<double>::infinity(), h->stream, h->knn_thr.p, h->knn_thr32.p);
    else launch_prm_pairs(h->dp, h->args, j0, j1, h->thr_conn, h->stream);
}
void launch_edges(oxhip_prm* h, const PrmArgs& a, uint32_t n_cand) {
    if (h->so3) launch_prm_so3_edges(h->dp, a, n_cand, h->stream);
    else launch_prm_edges(h->dp, a, n_cand, h->stream);
}
// what "near the start" is compared with: SO(3) compares the distance with the radius itself, R^n d2 with its squared threshold
double near_threshold(const oxhip_prm* h) { return h->so3 ? h->cfg.connection_radius : h->thr_conn; }
void launch_query(oxhip_prm* h) {
    DevParams qdp = h->dp;   // the start may lie anywhere: widen the filter's absolute margin for this launch
    for (uint32_t k = 0; k < h->cfg.dim; ++k) qdp.filt_abs = std::fmax(qdp.filt_abs, 1e-9 * std::fabs(h->query.start[k]));
    launch_prm_query(h->so3, qdp, h->args, h->n, h->query, near_threshold(h), h->flags.p, h->start_valid.p, h->stream);
}
void launch_batch_flags(oxhip_prm* h, const PrmBatchArgs& b) { launch_prm_batch_flags(h->so3, h->dp, b, near_threshold(h), h->stream); }
// a planted roadmap's fl32 shadow, which the R^n pair search screens with (the SO(3) pair search screens nothing)
void launch_planted_shadow(oxhip_prm* h, uint32_t n) {
    if (!h->so3) launch_prm_shadow(h->ms.p, h->ms32.p, (uint64_t)n * h->cfg.dim, h->stream);
}
// the re-check's pair list: R^n (entry, u, v) for its own check kernel; SO(3) construction's candidate layout, with a key array
// and a counter of the re-check's own, for construction's edge kernel
int32_t reserve_reval_pairs(oxhip_prm* h, uint32_t pair_cap) {
    if (!h->so3) { HIP_TRY(h->rv_pairs.reserve(pair_cap)); return OXHIP_OK; }
    HIP_TRY(h->rv_cand.reserve(pair_cap)); HIP_TRY(h->rv_keys.reserve(2 * (size_t)pair_cap)); HIP_TRY(h->rv_state.reserve(1));
    HIP_TRY(hipMemsetAsync(h->rv_state.p, 0, sizeof(PrmState), h->stream));
    return OXHIP_OK;
}
uint2* reval_cand(oxhip_prm* h) { return h->so3 ? h->rv_cand.p : nullptr; }   // (the emit launcher fills rv_pairs when this is null)
// check_motion(from = u, to = v) per pair of the list; a valid one keeps its two entries
int32_t launch_reval_edges(oxhip_prm* h, uint32_t n_pairs, uint32_t n, uint32_t n_old) {
    if (!h->so3) {
        launch_prm_reval_check(h->dp, h->ms.p, h->offsets.p, h->nbrs.p, n, n_old, h->rv_pairs.p, n_pairs, h->rv_keep.p, h->stream);
    } else if (n_pairs) {
        PrmArgs a = h->args;   // construction's kernel, the re-check's buffers: nothing of construction's workspace is touched
        a.cand = h->rv_cand.p; a.keys = h->rv_keys.p; a.state = h->rv_state.p;
        launch_edges(h, a, n_pairs);   // both directed keys of every valid pair
        HIP_TRY(hipGetLastError());
        launch_prm_reval_keys(h->rv_keys.p, h->rv_state.p, 2 * n_pairs, prm_key_shift(h->args.cap), h->offsets.p, h->nbrs.p, n, h->rv_keep.p,
                              h->stream);
    }
    return OXHIP_OK;
}
// what a goal's radius is compared with: SO(3) compares the distance with the radius itself, R^n d2 with its squared threshold
double goal_threshold(const oxhip_prm* h, double radius) { return h->so3 ? radius : sqrt_le_threshold(radius); }

// `count` coordinates of starts and of goal centres: what oxhip_prm_set_problem accepts
int32_t check_query_points(const double* starts, const double* goal_centres, size_t count) {
    for (size_t k = 0; k < count; ++k)
        if (!(std::fabs(starts[k]) <= kMaxMagnitude) || !(std::fabs(goal_centres[k]) <= kMaxMagnitude))
            return fail(OXHIP_ERR_BAD_ARG, "start / goal centre not finite or beyond 1e150");
    return OXHIP_OK;
}

int32_t set_query(oxhip_prm* h, const double* start, const double* goal_centre, double goal_radius) {
    const uint32_t dim = h->cfg.dim;
    OX_TRY(check_query_points(start, goal_centre, dim));
    h->query = PrmQuery{};
    std::memcpy(h->query.start, start, dim * sizeof(double));
    std::memcpy(h->query.goal_c, goal_centre, dim * sizeof(double));
    h->query.goal_thr = goal_threshold(h, goal_radius);
    return OXHIP_OK;
}

// what belongs to the roadmap as it was: gone whenever the roadmap is cleared, replaced (set_roadmap) or pruned (revalidate)
void drop_derived(oxhip_prm* h) {
    h->host_copy = false;
    h->h_offsets.clear();
    h->h_nbrs.clear();
    h->h_states.clear();
    h->start_conn.clear();
    h->goal_idx.clear();
    h->batch_valid = false;   // the batch's results are about the roadmap that just went
    h->w_valid = false;       // and so are the edge weights
    h->cc_valid = false;      // and the component labels
}

void clear_roadmap(oxhip_prm* h) {
    h->n = 0;
    h->n_keys = 0;
    h->n_samples = 0;
    h->redraw_batches = 0;
    h->pos_valid = false;   // (setup, set_roadmap: the stream position belonged to the roadmap that went)
    drop_derived(h);
}

// One round of the space's parallel sampler from stream word st.draws on.  R^n: m samples.  SO(3) (prm_so3.hip): m rejection
// attempts, attempt a at stream word pos0 + 4 a.
int32_t sample_round(oxhip_prm* h, const PrmState& st, uint32_t m) {
    if (h->so3) {
        HIP_TRY(h->spec_abits.reserve((m + 63) / 64)); HIP_TRY(h->spec_acnt.reserve((m + 63) / 64));
        PrmSo3Spec sp{};
        sp.pos0 = st.draws; sp.m = m;
        sp.tmp = h->spec_tmp.p; sp.vbits = h->spec_vbits.p; sp.abits = h->spec_abits.p; sp.voff = h->spec_off.p; sp.acnt = h->spec_acnt.p;
        sp.redraw_flag = h->spec_flag.p; sp.result = h->state.p;
        launch_prm_so3_sample(h->dp, h->args, sp, st.n_milestones, h->stream);
    } else {
        PrmSpec sp{};
        sp.pos0 = st.draws; sp.m = m;
        sp.tmp = h->spec_tmp.p; sp.vbits = h->spec_vbits.p; sp.wave_off = h->spec_off.p;
        sp.redraw_flag = h->spec_flag.p; sp.result = h->state.p;   // the scan kernel advances the device state
        launch_prm_sample_spec(h->dp, h->args, sp, st.n_milestones, h->stream);
    }
    HIP_TRY(hipGetLastError());
    return OXHIP_OK;
}

// A round whose flag came back set.  R^n: rand's range sampler would have rejected a draw somewhere in it (about as likely as a
// 2^-52 event): put the state back and replay this window in order with the sequential kernel, exact for any bounds.  SO(3):
// random_range(-1.0..1.0) cannot draw again (its largest value is 1 - 2^-51), so the word positions would be wrong: refused, never shifted.
int32_t flagged_round(oxhip_prm* h, PrmState& st, uint32_t m) {
    if (h->so3) return fail(OXHIP_ERR_HIP, "SO(3) sampler: random_range(-1.0..1.0) drew again, which cannot happen; round refused");
    OX_TRY(write_state(h, st));
    h->args.max_samples = st.n_samples + m;
    launch_prm_sample(h->dp, h->args, h->stream);
    HIP_TRY(hipGetLastError());
    return read_state(h, st);
}

// Draw samples until `target` milestones exist or `max_samples` were drawn: rounds of the parallel sampler, sized by the observed
// rate of milestones per sample (SO(3): per attempt; its kernel stops at args.max_samples itself, so its rounds are not clamped).
int32_t sample_until(oxhip_prm* h, PrmState& st, uint32_t target, uint64_t max_samples) {
    constexpr uint64_t kRoundMax = 1ull << 22;
    const bool so3 = h->so3;
    h->args.n_target = target;
    if (so3) h->args.max_samples = max_samples;
    while (st.n_milestones < target && st.n_samples < max_samples) {
        const uint32_t need = target - st.n_milestones;
        uint64_t want = std::min((uint64_t)((double)need / h->valid_rate * 1.02) + 256, kRoundMax);
        if (!so3) want = std::min(want, max_samples - st.n_samples);
        const uint32_t m = (uint32_t)want, nw = (m + 63) / 64;
        HIP_TRY(h->spec_tmp.reserve((size_t)m * h->cfg.dim)); HIP_TRY(h->spec_flag.reserve(1));   // (SO(3): dim is 4)
        HIP_TRY(h->spec_vbits.reserve(nw)); HIP_TRY(h->spec_off.reserve(nw));
        HIP_TRY(hipMemsetAsync(h->spec_flag.p, 0, sizeof(uint32_t), h->stream));
        OX_TRY(sample_round(h, st, m));
        PrmState after{};
        uint32_t flag = 0;
        HIP_TRY(hipMemcpyAsync(&after, h->state.p, sizeof(PrmState), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(&flag, h->spec_flag.p, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        if (flag != 0) { OX_TRY(flagged_round(h, st, m)); continue; }
        const double got = (double)(after.n_milestones - st.n_milestones), drawn = so3 ? (double)m : (double)(after.n_samples - st.n_samples);
        h->valid_rate = std::max(so3 ? 1e-6 : 1.0 / 64.0, std::min(1.0, (got + 1.0) / (drawn + 1.0)));
        st = after;
    }
    return OXHIP_OK;
}

// |dot| bands of "distance < r" (DESIGN.md section 15).  distance = |dot| > 1 - 1e-9 ? 0 : ox_acos(|dot|), ox_acos within
// delta = 2^-52 relative of the true acos (below one ulp; the CPU suite checks 2^-50 against libm), acos
// strictly decreasing.  hi >= cos(r (1 - 2^-40)): |dot| > hi gives ox_acos < acos(hi) (1 + delta) < r, or the 1 - 1e-9 shortcut's 0.
// lo <= cos(r (1 + 2^-40)) and lo <= 1 - 1e-9: |dot| < lo gives ox_acos > acos(lo) (1 - delta) > r.  libm's cos is within one ulp
// (2^-53 here) and each margin operation rounds once, both far inside the 2^-50 added.  Between lo and hi: the exact distance.
// No distance exceeds fl(PI / 2) (ox_acos(0) and, below |dot| 2^-55, pio2_hi - (x - pio2_lo) rounds to pio2_hi), so a radius
// above it takes every pair: hi = lo = -1.  r <= 0 takes none (the caller skips the search).
void so3_radius_bands(double r, double& lo, double& hi) {
    const double pio2 = 1.57079632679489655800e+00;
    if (!(r <= pio2)) { lo = hi = -1.0; return; }
    hi = std::cos(r * (1.0 - 0x1p-40)) + 0x1p-50;
    lo = std::fmin(std::cos(r * (1.0 + 0x1p-40)) - 0x1p-50, 1.0 - 1e-9);
}

// host copy of the roadmap for get_roadmap and the breadth-first query (once per construction)
int32_t fetch_roadmap(oxhip_prm* h) {
    if (h->host_copy) return OXHIP_OK;
    const uint32_t n = h->n, n_keys = h->n_keys;
    h->h_offsets.assign((size_t)n + 1, 0);
    h->h_nbrs.assign(n_keys, 0);
    h->h_states.assign((size_t)n * h->cfg.dim, 0.0);
    if (n) {
        HIP_TRY(hipMemcpyAsync(h->h_offsets.data(), h->offsets.p, ((size_t)n + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        if (n_keys) HIP_TRY(hipMemcpyAsync(h->h_nbrs.data(), h->nbrs.p, (size_t)n_keys * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(h->h_states.data(), h->ms.p, (size_t)n * h->cfg.dim * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    h->host_copy = true;
    return OXHIP_OK;
}

double elapsed_ms(hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? (double)ms : 0.0;
}

// ---- oxhip_prm_create in its steps
// Every refusal that precedes the choice of a device, in the order tests/golden/prm_create_refusals.json pins: pure host code.
// Returns the clamped fraction, res and (SO(3)) max_angle.
int32_t validate_prm_config(const oxhip_prm_config* cfg, double& fraction, double& res, double& so3_max_angle) {
    if (cfg->struct_size != sizeof(oxhip_prm_config)) return fail(OXHIP_ERR_BAD_ARG, "struct_size mismatch");
    if (cfg->max_milestones == 0 || cfg->max_milestones > (1u << 26)) return fail(OXHIP_ERR_BAD_ARG, "max_milestones must be in 1..2^26");
    if (std::isnan(cfg->connection_radius)) return fail(OXHIP_ERR_BAD_ARG, "connection_radius is NaN");
    if (cfg->space != OXHIP_SPACE_REAL_VECTOR && cfg->space != OXHIP_SPACE_SO3) return fail(OXHIP_ERR_BAD_ARG, "PRM space must be OXHIP_SPACE_REAL_VECTOR (0) or OXHIP_SPACE_SO3");
    fraction = cfg->lvs_fraction;
    if (cfg->space == OXHIP_SPACE_SO3) {
        OX_TRY(so3_space_resolution(cfg->dim, cfg->bounds, fraction, res, so3_max_angle));
        if (cfg->knn_k) return fail(OXHIP_ERR_BAD_ARG, "SO(3) PRM connects by radius only: knn_k must be 0");
        // no SO(3) motion is longer than PI / 2, whatever the radius
        if (std::fmin(cfg->connection_radius, 0.5 * 3.14159265358979323846) / res > 1e6)
            return fail(OXHIP_ERR_BAD_ARG, "more than 1e6 validity checks per edge");
    } else {
        OX_TRY(space_resolution(cfg->dim, cfg->bounds, fraction, res));
        // the longest motion PRM ever checks is shorter than the connection radius
        if (std::isfinite(cfg->connection_radius) && cfg->connection_radius / res > 1e6)
            return fail(OXHIP_ERR_BAD_ARG, "more than 1e6 validity checks per edge");
    }
    return OXHIP_OK;
}

// the midpoint filter's absolute margin (R^n): 1e-9 of the largest |coordinate| of the bounds and the sphere centres, at least 1e-9
void set_filter_margin(oxhip_prm* h, const std::vector<double>& centres) {
    h->maxabs = 1.0;
    for (uint32_t k = 0; k < 2 * h->cfg.dim; ++k) h->maxabs = std::fmax(h->maxabs, std::fabs(h->cfg.bounds[k]));
    for (double v : centres) h->maxabs = std::fmax(h->maxabs, std::fabs(v));
    h->dp.filt_abs = 1e-9 * h->maxabs;
}

void fill_prm_params(oxhip_prm* h, const oxhip_prm_config* cfg, double fraction, double res, double so3_max_angle) {
    h->cfg = *cfg;
    h->cfg.lvs_fraction = fraction;
    DevParams& dp = h->dp;
    dp.dim = cfg->dim; dp.res = res; dp.seed = cfg->seed;
    h->so3 = cfg->space == OXHIP_SPACE_SO3;
    if (h->so3) {   // the bounds are (cx, cy, cz, cw, max_angle); lo / hi / scale stay zero, and no coordinate enters the filter margin
        for (uint32_t k = 0; k < 4; ++k) dp.so3_centre[k] = cfg->bounds[k];
        dp.so3_max_angle = so3_max_angle;
        dp.space = OXHIP_SPACE_SO3;
        so3_radius_bands(cfg->connection_radius, h->so3_lo, h->so3_hi);
        dp.filt_abs = 1e-9 * h->maxabs;
    } else {
        for (uint32_t k = 0; k < cfg->dim; ++k) {
            dp.lo[k] = cfg->bounds[2 * k];
            dp.hi[k] = cfg->bounds[2 * k + 1];
            dp.scale[k] = dp.hi[k] - dp.lo[k];
        }
        set_filter_margin(h, {});
    }
    h->thr_conn = sqrt_lt_threshold(cfg->connection_radius);
}

// the stream, the events and the buffers that live as long as the handle; the first error wins
int32_t alloc_prm(oxhip_prm* h) {
    const uint32_t dim = h->cfg.dim, cap = ((h->cfg.max_milestones + 1023u) / 1024u) * 1024u;
    hipError_t e = hipSuccess;
    auto chk = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    chk(oxhip_stream_acquire(h->cfg.device, &h->stream));
    for (auto& ev : h->ev) chk(hipEventCreate(&ev));
    for (auto& ev : h->bev) chk(hipEventCreate(&ev));
    for (auto& ev : h->sev) chk(hipEventCreate(&ev));
    for (auto& ev : h->cev) chk(hipEventCreate(&ev));
    chk(h->ms.alloc((size_t)dim * cap));
    if (!h->so3) chk(h->ms32.alloc((size_t)dim * cap));   // (the SO(3) pair search screens nothing)
    chk(h->state.alloc(1));
    chk(h->flags.alloc(cap));
    chk(h->start_valid.alloc(1));
    chk(h->offsets.alloc((size_t)cap + 1));
    if (e != hipSuccess) return alloc_failed(e);
    h->args.ms = h->ms.p; h->args.ms32 = h->ms32.p; h->args.state = h->state.p;
    h->args.cap = cap; h->args.stream = h->cfg.stream;
    return OXHIP_OK;
}

// ---- oxhip_prm_construct_roadmap in its steps: each serves the milestones [n_done, n_now) of one round
// k-nearest variant: row j searches a radius expected to hold ~6 k earlier milestones -- the milestones are uniform over the valid
// part of the box (fraction n / n_samples of its volume V): count(r) ~ j c_D r^D / (V f) -- so that its k nearest are almost surely
// among the hits; a row that falls short gets the exact search afterwards (knn_select)
int32_t knn_row_radii(oxhip_prm* h, const PrmState& st, uint32_t n_done, uint32_t n_now) {
    const uint32_t dim = h->cfg.dim;
    double vol = 1.0;
    for (uint32_t k2 = 0; k2 < dim; ++k2) vol *= h->cfg.bounds[2 * k2 + 1] - h->cfg.bounds[2 * k2];
    const double frac = st.n_samples ? std::fmin(1.0, (double)n_now / (double)st.n_samples) : 1.0;
    const double c_d = std::pow(3.14159265358979323846, 0.5 * dim) / std::tgamma(0.5 * dim + 1.0);
    const double want = 6.0 * h->cfg.knn_k;
    std::vector<double> thr(h->args.cap, std::numeric_limits<double>::infinity());
    std::vector<float> thr32(h->args.cap, std::numeric_limits<float>::infinity());
    for (uint32_t j = n_done; j < n_now; ++j) {
        if ((double)j <= want) continue;   // few earlier milestones: all of them are candidates
        const double rd = want * vol * frac / (c_d * (double)j);
        const double r = std::pow(rd, 1.0 / dim);
        thr[j] = r * r;
        thr32[j] = prm_screen_threshold(h->dp, thr[j]);
    }
    HIP_TRY(h->knn_thr.reserve(h->args.cap)); HIP_TRY(h->knn_thr32.reserve(h->args.cap));
    HIP_TRY(hipMemcpyAsync(h->knn_thr.p, thr.data(), thr.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->knn_thr32.p, thr32.data(), thr32.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return OXHIP_OK;
}

// pairs (j in [n_done, n_now), i < j) within the connection radius, into h->cand; st.n_cand counts them
int32_t find_pairs(oxhip_prm* h, PrmState& st, uint32_t n_done, uint32_t n_now) {
    if (h->cand.n == 0) HIP_TRY(h->cand.alloc(std::min<size_t>(std::max<size_t>(1u << 20, (size_t)64 * h->cfg.max_milestones), (size_t)1 << 28)));
    for (;;) {
        h->args.cand = h->cand.p;
        h->args.cand_cap = (uint32_t)h->cand.n;
        st.n_cand = 0;
        OX_TRY(write_state(h, st));
        HIP_TRY(hipEventRecord(h->ev[2], h->stream));
        launch_pairs(h, n_done, n_now);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(h->ev[3], h->stream));
        PrmState s2{};
        OX_TRY(read_state(h, s2));
        h->t_ms[1] += elapsed_ms(h->ev[2], h->ev[3]);
        st.n_cand = s2.n_cand;
        if (st.n_cand <= h->args.cand_cap) break;
        // candidate buffer too small: the kernel kept counting, so the exact need is known; run again
        if (st.n_cand > 0x7FFFFFFFull) return fail(OXHIP_ERR_CAPACITY, "more than 2^31 in-radius pairs in one round");
        HIP_TRY(h->cand.alloc((size_t)st.n_cand));
    }
    h->n_candidates += st.n_cand;
    return OXHIP_OK;
}

// k-nearest variant: each row's k nearest among its candidates (sorted by (j, i)), the exact search for rows that fell short.
// The selected pairs replace the candidates as what the edge step reads: `pairs` and st.n_cand.
int32_t knn_select(oxhip_prm* h, PrmState& st, uint32_t n_done, uint32_t n_now, uint2*& pairs) {
    const uint32_t nc = (uint32_t)st.n_cand, rows = n_now - n_done, knn_k = h->cfg.knn_k;
    HIP_TRY(h->knn_keys.reserve(nc + 1)); HIP_TRY(h->knn_sorted.reserve(nc + 1)); HIP_TRY(h->knn_dist.reserve(nc + 1));
    HIP_TRY(h->knn_sel.reserve((size_t)rows * knn_k)); HIP_TRY(h->knn_failed.reserve(rows)); HIP_TRY(h->knn_counters.reserve(2));
    size_t tb = 0;
    if (nc) {
        HIP_TRY(prm_sort_keys(nullptr, tb, h->knn_keys.p, h->knn_sorted.p, nc, h->args.cap, h->stream));
        HIP_TRY(h->sort_tmp.reserve(tb));
    }
    HIP_TRY(hipEventRecord(h->ev[2], h->stream));
    HIP_TRY(hipMemsetAsync(h->knn_counters.p, 0, 2 * sizeof(uint32_t), h->stream));
    launch_prm_knn_keys(h->args, nc, h->knn_keys.p, h->stream);
    if (nc) HIP_TRY(prm_sort_keys(h->sort_tmp.p, tb, h->knn_keys.p, h->knn_sorted.p, nc, h->args.cap, h->stream));
    launch_prm_knn_select(h->dp, h->args, h->knn_sorted.p, h->knn_dist.p, nc, n_done, n_now, knn_k, h->knn_sel.p, h->knn_counters.p,
                          h->knn_failed.p, h->stream);
    HIP_TRY(hipGetLastError());
    uint32_t cnt[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(cnt, h->knn_counters.p, sizeof cnt, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (cnt[1]) {
        launch_prm_knn_brute(h->dp, h->args, h->knn_failed.p, cnt[1], knn_k, h->knn_sel.p, h->knn_counters.p, h->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(cnt, h->knn_counters.p, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->knn_failed_rows += cnt[1];
    }
    HIP_TRY(hipEventRecord(h->ev[3], h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->t_ms[1] += elapsed_ms(h->ev[2], h->ev[3]);
    st.n_cand = cnt[0];
    pairs = h->knn_sel.p;
    return OXHIP_OK;
}

// room for the keys this round can add, at most 2 per pair: growth keeps the keys of the rounds before
int32_t reserve_keys(oxhip_prm* h, const PrmState& st) {
    const uint64_t need = (uint64_t)st.n_keys + 2ull * st.n_cand;
    if (need > 0xFFFFFFFFull) return fail(OXHIP_ERR_CAPACITY, "more than 2^32 directed edges");
    if (need <= h->keys.n) return OXHIP_OK;
    DevBuf<uint64_t> bigger;
    HIP_TRY(bigger.alloc(std::max<size_t>((size_t)need, h->keys.n * 2)));
    if (st.n_keys) HIP_TRY(hipMemcpyAsync(bigger.p, h->keys.p, (size_t)st.n_keys * sizeof(uint64_t), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    std::swap(bigger.p, h->keys.p); std::swap(bigger.n, h->keys.n);
    h->args.keys = h->keys.p;
    return OXHIP_OK;
}

// check_motion per pair of `pairs`; the kernel appends the keys of the edges and st comes back with their count
int32_t check_edges(oxhip_prm* h, PrmState& st, uint2* pairs) {
    PrmArgs a = h->args;
    a.cand = pairs;
    HIP_TRY(hipEventRecord(h->ev[2], h->stream));
    launch_edges(h, a, (uint32_t)st.n_cand);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev[3], h->stream));
    OX_TRY(read_state(h, st));
    h->t_ms[2] += elapsed_ms(h->ev[2], h->ev[3]);
    return OXHIP_OK;
}

// sort the directed keys -> every node's neighbours in ascending order (the reference's `edges`), as CSR
int32_t build_csr(oxhip_prm* h, uint32_t n, uint32_t n_keys) {
    size_t tmp_bytes = 0;
    if (n_keys) {
        // (re)size the sort's buffers before the timed region: hipMalloc is a blocking call
        HIP_TRY(h->keys_sorted.reserve(n_keys)); HIP_TRY(h->nbrs.reserve(n_keys));
        HIP_TRY(prm_sort_keys(nullptr, tmp_bytes, h->keys.p, h->keys_sorted.p, n_keys, h->args.cap, h->stream));
        HIP_TRY(h->sort_tmp.reserve(tmp_bytes));
    }
    HIP_TRY(hipEventRecord(h->ev[4], h->stream));
    if (n_keys) {
        HIP_TRY(prm_sort_keys(h->sort_tmp.p, tmp_bytes, h->keys.p, h->keys_sorted.p, n_keys, h->args.cap, h->stream));
        launch_prm_csr(h->keys_sorted.p, n_keys, n, h->args.cap, h->offsets.p, h->nbrs.p, h->stream);
        HIP_TRY(hipGetLastError());
    } else {
        HIP_TRY(hipMemsetAsync(h->offsets.p, 0, ((size_t)n + 1) * sizeof(uint32_t), h->stream));
    }
    HIP_TRY(hipEventRecord(h->ev[5], h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->t_ms[3] = elapsed_ms(h->ev[4], h->ev[5]);
    return OXHIP_OK;
}

// start validity, start connections and goal milestones of h->query (prm.rs:243-264), on the device
int32_t query_sets(oxhip_prm* h, std::vector<uint8_t>& flags) {
    const uint32_t n = h->n;
    uint32_t start_valid = 0;
    HIP_TRY(hipEventRecord(h->ev[0], h->stream));
    launch_query(h);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev[1], h->stream));
    flags.assign(n, 0);
    HIP_TRY(hipMemcpyAsync(flags.data(), h->flags.p, n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(&start_valid, h->start_valid.p, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->t_ms[4] = elapsed_ms(h->ev[0], h->ev[1]);
    if (!start_valid) return fail(OXHIP_ERR_INVALID_START_STATE, "start state is in collision");  // prm.rs:243-246
    for (uint32_t i = 0; i < n; ++i) {
        if (flags[i] & 1) h->start_conn.push_back(i);   // prm.rs:249-256
        if (flags[i] & 2) h->goal_idx.push_back(i);     // prm.rs:259-264
    }
    return OXHIP_OK;
}

}  // namespace

extern "C" {

int32_t oxhip_prm_create(const oxhip_prm_config* cfg, oxhip_prm** out) {
    if (!cfg || !out) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    *out = nullptr;
    double fraction = 0.0, res = 0.0, so3_max_angle = 0.0;
    OX_TRY(validate_prm_config(cfg, fraction, res, so3_max_angle));
    OX_TRY(select_device(cfg->device));
    std::unique_ptr<oxhip_prm, decltype(&oxhip_prm_destroy)> h(new oxhip_prm(), oxhip_prm_destroy);   // (an early return destroys it)
    fill_prm_params(h.get(), cfg, fraction, res, so3_max_angle);
    OX_TRY(alloc_prm(h.get()));
    *out = h.release();
    return OXHIP_OK;
}

int32_t oxhip_prm_destroy(oxhip_prm* h) {
    if (!h) return OXHIP_OK;
    (void)hipSetDevice(h->cfg.device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (auto& ev : h->ev) if (ev) (void)hipEventDestroy(ev);
    for (auto& ev : h->bev) if (ev) (void)hipEventDestroy(ev);
    for (auto& ev : h->sev) if (ev) (void)hipEventDestroy(ev);
    for (auto& ev : h->cev) if (ev) (void)hipEventDestroy(ev);
    if (h->stream) oxhip_stream_release(h->cfg.device, h->stream);
    delete h;
    return OXHIP_OK;
}

int32_t oxhip_prm_set_spheres(oxhip_prm* h, const double* centres, const double* radii, uint32_t n) {
    if (!h || (n && (!centres || !radii))) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    OX_TRY(select_device(h->cfg.device));
    const uint32_t dim = h->cfg.dim;
    std::vector<double> c((size_t)dim * n), thr(n);
    for (uint32_t j = 0; j < n; ++j) {
        for (uint32_t k = 0; k < dim; ++k) {
            double v = centres[(size_t)j * dim + k];
            if (!(std::fabs(v) <= kMaxMagnitude)) return fail(OXHIP_ERR_BAD_ARG, "sphere centre not finite / too large");
            c[(size_t)k * n + j] = v;  // SoA [dim][n]
        }
        thr[j] = sqrt_le_threshold(radii[j]);
    }
    OX_TRY(upload(h->sph_c, c, h->stream));
    OX_TRY(upload(h->sph_thr, thr, h->stream));
    OX_TRY(upload(h->sph_r, std::vector<double>(radii, radii + n), h->stream));
    h->dp.n_spheres = n; h->dp.sph_c = h->sph_c.p; h->dp.sph_thr = h->sph_thr.p; h->dp.sph_r = h->sph_r.p;
    if (!h->so3) set_filter_margin(h, c);   // (cones: distance(centre, q) > radius, compared with sph_r itself; no filter)
    return OXHIP_OK;
}

int32_t oxhip_prm_set_boxes(oxhip_prm* h, const double* lo, const double* hi, uint32_t n) {
    if (!h || (n && (!lo || !hi))) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    if (h->so3) return fail(OXHIP_ERR_BAD_ARG, "SO(3) PRM takes cones (oxhip_prm_set_spheres with 4-wide centres), not boxes");
    OX_TRY(select_device(h->cfg.device));
    const uint32_t dim = h->cfg.dim;
    std::vector<double> l((size_t)dim * n), u((size_t)dim * n);
    for (uint32_t j = 0; j < n; ++j)
        for (uint32_t k = 0; k < dim; ++k) {
            l[(size_t)k * n + j] = lo[(size_t)j * dim + k];
            u[(size_t)k * n + j] = hi[(size_t)j * dim + k];
        }
    OX_TRY(upload(h->box_lo, l, h->stream));
    OX_TRY(upload(h->box_hi, u, h->stream));
    h->dp.n_boxes = n; h->dp.box_lo = h->box_lo.p; h->dp.box_hi = h->box_hi.p;
    return OXHIP_OK;
}

// Planner::setup (prm.rs:217-225)
int32_t oxhip_prm_setup(oxhip_prm* h, const double* start, const double* goal_centre, double goal_radius) {
    if (!h || !start || !goal_centre) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    OX_TRY(select_device(h->cfg.device));
    OX_TRY(set_query(h, start, goal_centre, goal_radius));
    clear_roadmap(h);  // self.roadmap.clear()
    PrmState st{};
    OX_TRY(write_state(h, st));
    h->is_setup = true;
    return OXHIP_OK;
}

// set_problem_definition (prm.rs:88-90): the roadmap is kept
int32_t oxhip_prm_set_problem(oxhip_prm* h, const double* start, const double* goal_centre, double goal_radius) {
    if (!h || !start || !goal_centre) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    return set_query(h, start, goal_centre, goal_radius);
}

// construct_roadmap (prm.rs:96-154)
int32_t oxhip_prm_construct_roadmap(oxhip_prm* h) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (!h->is_setup) return fail(OXHIP_ERR_PLANNER_UNINITIALISED, "setup() was not called");  // prm.rs:97-104
    if (h->n != 0) return OXHIP_OK;  // prm.rs:106-113: "Roadmap already constructed"
    OX_TRY(select_device(h->cfg.device));
    const auto t0 = std::chrono::steady_clock::now();
    const bool has_timeout = h->cfg.timeout > 0.0 && std::isfinite(h->cfg.timeout);
    const uint32_t n_max = h->cfg.max_milestones, knn_k = h->cfg.knn_k;
    // 0 = "unlimited", which still has to end when (almost) no sample is valid: 4096 draws per requested milestone
    const uint64_t max_samples = h->cfg.max_samples ? h->cfg.max_samples : 4096ull * n_max + (1ull << 22);
    for (double& t : h->t_ms) t = 0.0;
    h->n_candidates = 0;
    h->knn_failed_rows = 0;
    PrmState st{};
    OX_TRY(write_state(h, st));
    h->valid_rate = 1.0;
    // without a wall clock the roadmap is built in one round; with one, in doubling rounds with the
    // clock read in between (the reference reads it before every sample, prm.rs:118)
    uint32_t target = has_timeout ? std::min<uint32_t>(n_max, 4096u) : n_max;
    uint32_t n_done = 0;  // milestones whose pairs are already connected
    for (;;) {
        HIP_TRY(hipEventRecord(h->ev[0], h->stream));
        OX_TRY(sample_until(h, st, target, max_samples));
        HIP_TRY(hipEventRecord(h->ev[1], h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->t_ms[0] += elapsed_ms(h->ev[0], h->ev[1]);
        const uint32_t n_now = st.n_milestones;
        // thr_conn >= 0 <=> connection_radius > 0 (sqrt_lt_threshold; NaN was refused), in either space: a radius <= 0 takes no pair
        if (n_now > n_done && n_now >= 2 && (h->thr_conn >= 0.0 || knn_k)) {
            if (knn_k) OX_TRY(knn_row_radii(h, st, n_done, n_now));
            OX_TRY(find_pairs(h, st, n_done, n_now));
            uint2* pairs = h->cand.p;
            if (knn_k) OX_TRY(knn_select(h, st, n_done, n_now, pairs));
            OX_TRY(reserve_keys(h, st));
            OX_TRY(check_edges(h, st, pairs));
        }
        n_done = n_now;
        if (n_now < target) break;                       // max_samples exhausted
        if (n_now >= n_max) break;
        if (has_timeout && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > h->cfg.timeout)
            break;                                       // prm.rs:118-120
        target = target > n_max / 2 ? n_max : target * 2;
    }
    OX_TRY(build_csr(h, st.n_milestones, st.n_keys));
    h->n_keys = st.n_keys;
    h->w_valid = false;     // the edge weights of the roadmap before this one
    h->cc_valid = false;    // and its component labels
    h->host_copy = false;   // fetched by the first get_roadmap / solve
    h->n = st.n_milestones;
    h->n_samples = st.n_samples;
    h->redraw_batches = st.redraw_batches;
    h->pos_valid = true; h->pos_stream = h->cfg.stream; h->pos_draws = st.draws;   // where oxhip_prm_grow_roadmap continues
    return OXHIP_OK;
}

int32_t oxhip_prm_knn_exact_rows(oxhip_prm* h, uint32_t* rows) {
    if (!h || !rows) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    *rows = h->knn_failed_rows;
    return OXHIP_OK;
}

int32_t oxhip_prm_get_sizes(oxhip_prm* h, uint32_t* n_milestones, uint64_t* n_edge_entries, uint64_t* n_samples) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (n_milestones) *n_milestones = h->n;
    if (n_edge_entries) *n_edge_entries = h->n_keys;
    if (n_samples) *n_samples = h->n_samples;
    return OXHIP_OK;
}

// get_roadmap (prm.rs:82-84)
int32_t oxhip_prm_get_roadmap(oxhip_prm* h, double* states, uint32_t cap_nodes, uint64_t* offsets, uint32_t* neighbours,
                              uint64_t cap_entries) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (h->n) {
        OX_TRY(select_device(h->cfg.device));
        OX_TRY(fetch_roadmap(h));
    }
    if ((states || offsets) && cap_nodes < h->n) return fail(OXHIP_ERR_CAPACITY, "roadmap buffers too small");
    if (neighbours && cap_entries < h->h_nbrs.size()) return fail(OXHIP_ERR_CAPACITY, "neighbour buffer too small");
    if (states && h->n) std::memcpy(states, h->h_states.data(), h->h_states.size() * sizeof(double));
    if (offsets) {
        for (uint32_t i = 0; i <= h->n; ++i) offsets[i] = h->h_offsets.empty() ? 0 : h->h_offsets[i];
    }
    if (neighbours && !h->h_nbrs.empty()) std::memcpy(neighbours, h->h_nbrs.data(), h->h_nbrs.size() * sizeof(uint32_t));
    return OXHIP_OK;
}

// Planner::solve (prm.rs:227-307)
int32_t oxhip_prm_solve(oxhip_prm* h, double timeout_s, double* path, uint32_t cap_states, uint32_t* len) {
    if (!h || !len) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    *len = 0;
    h->start_conn.clear();
    h->goal_idx.clear();
    if (!h->is_setup) return fail(OXHIP_ERR_PLANNER_UNINITIALISED, "setup() was not called");      // prm.rs:229-236
    if (h->n == 0) return fail(OXHIP_ERR_UNSAMPLED_STATE_SPACE, "construct_roadmap() left no milestones");  // prm.rs:239-241
    OX_TRY(select_device(h->cfg.device));
    OX_TRY(fetch_roadmap(h));
    std::vector<uint8_t> flags;
    OX_TRY(query_sets(h, flags));
    const auto t0 = std::chrono::steady_clock::now();
    const bool has_timeout = timeout_s > 0.0 && std::isfinite(timeout_s);
    std::vector<uint32_t> chain;   // goal milestone ... root connection
    const PrmBfs found = prm_bfs_path(h->h_offsets, h->h_nbrs, flags, h->start_conn, has_timeout ? timeout_s : std::numeric_limits<double>::infinity(), chain);
    if (found == PrmBfs::empty_set) return fail(OXHIP_ERR_NO_SOLUTION_FOUND, "start or goal does not connect to the roadmap");  // prm.rs:266-268
    h->t_ms[5] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (found == PrmBfs::timed_out) return fail(OXHIP_ERR_TIMEOUT, "graph search timed out");  // prm.rs:285-287
    if (found == PrmBfs::unreachable) return fail(OXHIP_ERR_NO_SOLUTION_FOUND, "goal is not reachable on the roadmap");  // prm.rs:304
    // [start] ++ (root connection ... goal milestone)
    const uint32_t dim = h->cfg.dim;
    *len = (uint32_t)chain.size() + 1;
    if (!path) return OXHIP_OK;
    if (*len > cap_states) return fail(OXHIP_ERR_CAPACITY, "path buffer too small");
    std::memcpy(path, h->query.start, dim * sizeof(double));
    for (size_t j = 0; j < chain.size(); ++j)
        std::memcpy(path + (j + 1) * dim, h->h_states.data() + (size_t)chain[chain.size() - 1 - j] * dim, dim * sizeof(double));
    return OXHIP_OK;
}

int32_t oxhip_prm_get_query_sets(oxhip_prm* h, uint32_t* start_connections, uint32_t cap_start, uint32_t* n_start,
                                 uint32_t* goal_indices, uint32_t cap_goal, uint32_t* n_goal) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (n_start) *n_start = (uint32_t)h->start_conn.size();
    if (n_goal) *n_goal = (uint32_t)h->goal_idx.size();
    if (start_connections) {
        if (cap_start < h->start_conn.size()) return fail(OXHIP_ERR_CAPACITY, "start_connections buffer too small");
        if (!h->start_conn.empty()) std::memcpy(start_connections, h->start_conn.data(), h->start_conn.size() * sizeof(uint32_t));
    }
    if (goal_indices) {
        if (cap_goal < h->goal_idx.size()) return fail(OXHIP_ERR_CAPACITY, "goal_indices buffer too small");
        if (!h->goal_idx.empty()) std::memcpy(goal_indices, h->goal_idx.data(), h->goal_idx.size() * sizeof(uint32_t));
    }
    return OXHIP_OK;
}

int32_t oxhip_prm_last_timing(oxhip_prm* h, double* phase_ms, uint64_t* n_candidates, uint32_t* redraw_batches) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (phase_ms) for (int i = 0; i < 6; ++i) phase_ms[i] = h->t_ms[i];
    if (n_candidates) *n_candidates = h->n_candidates;
    if (redraw_batches) *redraw_batches = h->redraw_batches;
    return OXHIP_OK;
}

}  // extern "C"

// ---- a batch of queries on the roadmap as it stands: prm.rs:243-307 per query, all of it on the device

namespace {

// the arguments of one round of the last batch: queries [q0, q0 + n_chunk) in the workspace rows [0, n_chunk)
PrmBatchArgs batch_args(oxhip_prm* h, uint32_t q0, uint32_t n_chunk, uint32_t res_cap) {
    PrmBatchArgs b{};
    b.ms = h->ms.p; b.offsets = h->offsets.p; b.nbrs = h->nbrs.p;
    b.starts = h->bd_starts.p; b.goals = h->bd_goals.p; b.goal_thr = h->bd_thr.p; b.filt = h->bd_filt.p;
    b.flags = h->bd_flags.p; b.start_valid = h->bd_start_valid.p; b.parent = h->bd_parent.p; b.queue = h->bd_queue.p;
    b.status = (int32_t*)h->bd_res.p; b.path_len = h->bd_res.p + res_cap; b.goal_node = (int32_t*)(h->bd_res.p + 2 * (size_t)res_cap);
    b.n_start = h->bd_res.p + 3 * (size_t)res_cap; b.n_goal = h->bd_res.p + 4 * (size_t)res_cap;
    b.n = h->n; b.stride = (h->n + 63u) & ~63u; b.dim = h->cfg.dim; b.q0 = q0; b.n_chunk = n_chunk;
    return b;
}

PrmShortestArgs shortest_args(oxhip_prm* h, int32_t mode) {
    PrmShortestArgs a{};
    a.w = h->w_edges.p; a.label = h->bd_label.p; a.stamp = h->bd_stamp.p; a.cost = h->bd_cost.p; a.rounds = h->bd_rounds.p;
    a.relaxed = h->bd_relaxed.p; a.mode = (uint32_t)mode;
    return a;
}

// the distances of the roadmap's CSR entries, once per roadmap (distance weights only)
int32_t ensure_edge_weights(oxhip_prm* h) {
    if (h->w_valid) return OXHIP_OK;
    HIP_TRY(h->w_edges.reserve(h->n_keys));
    HIP_TRY(hipEventRecord(h->sev[0], h->stream));
    launch_prm_shortest_weights(h->so3, h->cfg.dim, h->ms.p, h->offsets.p, h->nbrs.p, h->n, h->n_keys, h->w_edges.p, h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->sev[1], h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->short_ms[0] = elapsed_ms(h->sev[0], h->sev[1]);
    h->w_valid = true;
    return OXHIP_OK;
}

// bytes of a round's workspace per query and milestone: flag 1, parent 4, queue 4; label 8 and stamp 4 for the shortest-path search
uint64_t batch_bytes_per_node(int32_t mode) { return mode < 0 ? 9ull : 21ull; }

// one batch while it runs: its shape, and where a round's results land on the host before scatter_round files them per query
struct BatchRun {
    uint32_t Q = 0, chunk = 0, stride = 0, group = 0;
    int32_t mode = -1;   // < 0: the breadth-first search of prm.rs (oxhip_prm_solve_batch); 0, 1, 2: shortest paths with that weights mode
    PrmShortestArgs sa{};
    std::vector<uint32_t> res;   // [5][chunk] status, path_len, goal_node, n_start, n_goal
    std::vector<uint64_t> off;   // [chunk] first row of each query's path among the round's rows
};

// the checks, the host side of the batch (every query starts out OXHIP_ERR_TIMEOUT) and the upload of the queries
int32_t stage_batch(oxhip_prm* h, uint32_t Q, const double* starts, const double* goal_centres, const double* goal_radii, int32_t mode) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (Q && (!starts || !goal_centres || !goal_radii)) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    if (!h->is_setup) return fail(OXHIP_ERR_PLANNER_UNINITIALISED, "setup() was not called");      // prm.rs:229-236
    if (h->n == 0) return fail(OXHIP_ERR_UNSAMPLED_STATE_SPACE, "construct_roadmap() left no milestones");  // prm.rs:239-241
    const uint32_t dim = h->cfg.dim;
    OX_TRY(check_query_points(starts, goal_centres, (size_t)Q * dim));
    OX_TRY(select_device(h->cfg.device));
    h->batch_valid = false;
    h->batch_rounds = 0;
    h->batch_mode = mode;
    for (double& t : h->batch_ms) t = 0.0;
    for (double& t : h->short_ms) t = 0.0;
    h->b_cost.assign(mode < 0 ? 0 : Q, std::numeric_limits<double>::infinity());
    h->b_rounds.assign(mode < 0 ? 0 : Q, 0u);
    h->b_relaxed.assign(mode < 0 ? 0 : Q, 0ull);
    h->b_starts.assign(starts, starts + (size_t)Q * dim);
    h->b_goals.assign(goal_centres, goal_centres + (size_t)Q * dim);
    h->b_thr.resize(Q); h->b_filt.resize(Q);
    for (uint32_t q = 0; q < Q; ++q) {
        h->b_thr[q] = goal_threshold(h, goal_radii[q]);
        double f = h->dp.filt_abs;   // the start may lie anywhere: the filter's absolute margin with this start in play
        for (uint32_t k = 0; k < dim; ++k) f = std::fmax(f, 1e-9 * std::fabs(starts[(size_t)q * dim + k]));
        h->b_filt[q] = f;
    }
    h->b_status.assign(Q, OXHIP_ERR_TIMEOUT);
    h->b_goal_node.assign(Q, -1);
    h->b_len.assign(Q, 0); h->b_nstart.assign(Q, 0); h->b_ngoal.assign(Q, 0);
    h->b_off.assign((size_t)Q + 1, 0);
    h->b_nodes.clear(); h->b_rows.clear();
    if (!Q) return OXHIP_OK;
    HIP_TRY(h->bd_starts.reserve((size_t)Q * dim)); HIP_TRY(h->bd_goals.reserve((size_t)Q * dim));
    HIP_TRY(h->bd_thr.reserve(Q)); HIP_TRY(h->bd_filt.reserve(Q));
    HIP_TRY(hipMemcpyAsync(h->bd_starts.p, h->b_starts.data(), (size_t)Q * dim * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->bd_goals.p, h->b_goals.data(), (size_t)Q * dim * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->bd_thr.p, h->b_thr.data(), (size_t)Q * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->bd_filt.p, h->b_filt.data(), (size_t)Q * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return OXHIP_OK;
}

// The size of a round -- 9 bytes per query and milestone (21 for shortest paths), sized to keep the workspace within 1 GiB -- and
// every buffer a round of that size needs; distance weights: the roadmap's edge weights, once per roadmap
int32_t reserve_batch_workspace(oxhip_prm* h, BatchRun& br, uint32_t chunk_queries) {
    br.stride = (h->n + 63u) & ~63u;
    uint32_t chunk = chunk_queries ? chunk_queries : (uint32_t)std::max<uint64_t>(1, (1ull << 30) / (batch_bytes_per_node(br.mode) * br.stride));
    br.chunk = chunk = std::min(std::min(chunk, br.Q), 65535u);
    const size_t cells = (size_t)chunk * br.stride;
    if (br.mode >= 0) {
        HIP_TRY(h->bd_label.reserve(cells)); HIP_TRY(h->bd_stamp.reserve(cells));
        HIP_TRY(h->bd_cost.reserve(chunk)); HIP_TRY(h->bd_rounds.reserve(chunk)); HIP_TRY(h->bd_relaxed.reserve(chunk));
    }
    if (br.mode == 0) OX_TRY(ensure_edge_weights(h));
    br.sa = shortest_args(h, br.mode);
    HIP_TRY(h->bd_flags.reserve(cells)); HIP_TRY(h->bd_parent.reserve(cells)); HIP_TRY(h->bd_queue.reserve(cells));
    HIP_TRY(h->bd_start_valid.reserve(chunk)); HIP_TRY(h->bd_off.reserve(chunk));
    HIP_TRY(h->bd_res.reserve(5 * (size_t)chunk));   // (the getters take bd_res.n / 5 as a round's row count: never below this one)
    br.group = prm_batch_group(h->n, h->n_keys);
    br.res.resize(5 * (size_t)chunk); br.off.resize(chunk);
    return OXHIP_OK;
}

// flags, initial labels, label rounds and tight levels of the queries of `b`; `timed`: a batch's round, which records its events between
int32_t launch_shortest(oxhip_prm* h, const PrmBatchArgs& b, const PrmShortestArgs& sa, uint32_t group, bool timed) {
    launch_batch_flags(h, b);
    launch_prm_shortest_init(h->so3, b, sa, h->stream);
    if (timed) HIP_TRY(hipEventRecord(h->bev[1], h->stream));
    launch_prm_shortest_labels(b, sa, group, h->stream);
    HIP_TRY(hipGetLastError());
    if (timed) HIP_TRY(hipEventRecord(h->sev[0], h->stream));
    launch_prm_shortest_levels(b, sa, group, h->stream);
    HIP_TRY(hipGetLastError());
    return OXHIP_OK;
}

// one round on the device: the query sets, the search, and its results copied into `br` (the search's own figures: to their queries)
int32_t run_round(oxhip_prm* h, BatchRun& br, const PrmBatchArgs& b) {
    const uint32_t c = b.n_chunk, q0 = b.q0;
    HIP_TRY(hipMemsetAsync(h->bd_parent.p, 0xFF, (size_t)c * br.stride * sizeof(uint32_t), h->stream));
    HIP_TRY(hipEventRecord(h->bev[0], h->stream));
    if (br.mode < 0) {
        launch_batch_flags(h, b);
        HIP_TRY(hipEventRecord(h->bev[1], h->stream));
        launch_prm_batch_search(b, br.group, h->stream);
        HIP_TRY(hipGetLastError());
    } else {
        OX_TRY(launch_shortest(h, b, br.sa, br.group, true));
    }
    HIP_TRY(hipEventRecord(h->bev[2], h->stream));
    HIP_TRY(hipMemcpyAsync(br.res.data(), h->bd_res.p, 5 * (size_t)br.chunk * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    if (br.mode >= 0) {
        HIP_TRY(hipMemcpyAsync(h->b_cost.data() + q0, h->bd_cost.p, (size_t)c * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(h->b_rounds.data() + q0, h->bd_rounds.p, (size_t)c * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(h->b_relaxed.data() + q0, h->bd_relaxed.p, (size_t)c * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipEventRecord(h->bev[3], h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->batch_ms[0] += elapsed_ms(h->bev[0], h->bev[1]);
    h->batch_ms[1] += elapsed_ms(h->bev[1], h->bev[2]);
    h->batch_ms[3] += elapsed_ms(h->bev[2], h->bev[3]);
    if (br.mode < 0) return OXHIP_OK;
    h->short_ms[2] += elapsed_ms(h->bev[1], h->sev[0]);
    h->short_ms[3] += elapsed_ms(h->sev[0], h->bev[2]);
    for (uint32_t i = 0; i < c; ++i)
        if ((int32_t)br.res[i] == OXHIP_ERR_HIP)   // (no query status is OXHIP_ERR_HIP otherwise)
            return fail(OXHIP_ERR_HIP, "shortest-path search: a label round or level cap was hit, which cannot happen");
    return OXHIP_OK;
}

// the round's results into the per-query vectors; returns the rows of the round's paths (br.off: where each begins among them)
uint64_t scatter_round(oxhip_prm* h, BatchRun& br, uint32_t q0, uint32_t c) {
    const size_t chunk = br.chunk;
    uint64_t rows = 0;
    const uint64_t row0 = h->b_off[q0];
    for (uint32_t i = 0; i < c; ++i) {
        h->b_status[q0 + i] = (int32_t)br.res[i];
        h->b_len[q0 + i] = br.res[chunk + i];
        h->b_goal_node[q0 + i] = (int32_t)br.res[2 * chunk + i];
        h->b_nstart[q0 + i] = br.res[3 * chunk + i];
        h->b_ngoal[q0 + i] = br.res[4 * chunk + i];
        br.off[i] = rows;
        rows += br.res[chunk + i];
        h->b_off[q0 + i + 1] = row0 + rows;
    }
    return rows;
}

// the `rows` path rows of the round, extracted on the device and appended to b_nodes / b_rows
int32_t extract_round_paths(oxhip_prm* h, const BatchRun& br, const PrmBatchArgs& b, uint64_t rows) {
    const uint32_t dim = h->cfg.dim;
    const uint64_t row0 = h->b_off[b.q0];
    HIP_TRY(h->bd_nodes.reserve((size_t)rows)); HIP_TRY(h->bd_rows.reserve((size_t)rows * dim));
    h->b_nodes.resize((size_t)(row0 + rows)); h->b_rows.resize((size_t)(row0 + rows) * dim);
    HIP_TRY(hipMemcpyAsync(h->bd_off.p, br.off.data(), (size_t)b.n_chunk * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipEventRecord(h->bev[4], h->stream));
    launch_prm_batch_paths(b, h->bd_off.p, h->bd_nodes.p, h->bd_rows.p, h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->bev[5], h->stream));
    HIP_TRY(hipMemcpyAsync(h->b_nodes.data() + row0, h->bd_nodes.p, (size_t)rows * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(h->b_rows.data() + (size_t)row0 * dim, h->bd_rows.p, (size_t)rows * dim * sizeof(double), hipMemcpyDeviceToHost,
                           h->stream));
    HIP_TRY(hipEventRecord(h->bev[6], h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->batch_ms[2] += elapsed_ms(h->bev[4], h->bev[5]);
    h->batch_ms[3] += elapsed_ms(h->bev[5], h->bev[6]);
    return OXHIP_OK;
}

int32_t solve_batch_common(oxhip_prm* h, uint32_t n_queries, const double* starts, const double* goal_centres, const double* goal_radii,
                           double timeout_s, uint32_t chunk_queries, int32_t mode, int32_t* status_out) {
    const auto t0 = std::chrono::steady_clock::now();
    const bool has_timeout = timeout_s > 0.0 && std::isfinite(timeout_s);
    OX_TRY(stage_batch(h, n_queries, starts, goal_centres, goal_radii, mode));
    BatchRun br;
    br.Q = n_queries; br.mode = mode;
    if (br.Q) {
        OX_TRY(reserve_batch_workspace(h, br, chunk_queries));
        uint32_t answered = 0;
        for (uint32_t q0 = 0; q0 < br.Q; q0 += br.chunk) {
            // the clock is read between rounds: the queries of the rounds not begun keep OXHIP_ERR_TIMEOUT
            if (q0 && has_timeout && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s) break;
            const uint32_t c = std::min(br.chunk, br.Q - q0);
            const PrmBatchArgs b = batch_args(h, q0, c, br.chunk);
            OX_TRY(run_round(h, br, b));
            const uint64_t rows = scatter_round(h, br, q0, c);
            if (rows) OX_TRY(extract_round_paths(h, br, b, rows));
            ++h->batch_rounds;
            answered = q0 + c;
        }
        for (uint32_t q = answered + 1; q <= br.Q; ++q) h->b_off[q] = h->b_off[answered];   // (the rounds not begun add no rows)
    }
    if (mode >= 0) { h->short_ms[1] = h->batch_ms[0]; h->short_ms[4] = h->batch_ms[2]; h->short_ms[5] = h->batch_ms[3]; }
    h->batch_valid = true;
    if (status_out) for (uint32_t q = 0; q < br.Q; ++q) status_out[q] = h->b_status[q];
    return OXHIP_OK;
}

}  // namespace

extern "C" {

int32_t oxhip_prm_solve_batch(oxhip_prm* h, uint32_t n_queries, const double* starts, const double* goal_centres, const double* goal_radii,
                              double timeout_s, uint32_t chunk_queries, int32_t* status_out) {
    return solve_batch_common(h, n_queries, starts, goal_centres, goal_radii, timeout_s, chunk_queries, -1, status_out);
}

int32_t oxhip_prm_solve_batch_shortest(oxhip_prm* h, uint32_t n_queries, const double* starts, const double* goal_centres,
                                       const double* goal_radii, double timeout_s, uint32_t chunk_queries, uint32_t weights, int32_t* status_out) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (weights > 2u) return fail(OXHIP_ERR_BAD_ARG, "weights must be 0 (distance), 1 (unit) or 2 (zero)");
    return solve_batch_common(h, n_queries, starts, goal_centres, goal_radii, timeout_s, chunk_queries, (int32_t)weights, status_out);
}

int32_t oxhip_prm_batch_get_costs(oxhip_prm* h, double* cost) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (!h->batch_valid) return fail(OXHIP_ERR_UNSAMPLED_STATE_SPACE, "no batch was solved on this roadmap");
    if (h->batch_mode < 0) return fail(OXHIP_ERR_BAD_ARG, "the last batch was not a shortest-path batch");
    if (cost && !h->b_cost.empty()) std::memcpy(cost, h->b_cost.data(), h->b_cost.size() * sizeof(double));
    return OXHIP_OK;
}

int32_t oxhip_prm_batch_get_labels(oxhip_prm* h, uint32_t query, double* cost, uint32_t* hops, uint32_t* parent, uint32_t cap) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (!h->batch_valid) return fail(OXHIP_ERR_UNSAMPLED_STATE_SPACE, "no batch was solved on this roadmap");
    if (h->batch_mode < 0) return fail(OXHIP_ERR_BAD_ARG, "the last batch was not a shortest-path batch");
    if (query >= h->b_status.size()) return fail(OXHIP_ERR_BAD_ARG, "query index beyond the last batch");
    const uint32_t n = h->n;
    if ((cost || hops || parent) && cap < n) return fail(OXHIP_ERR_CAPACITY, "label buffers too small");
    if (!cost && !hops && !parent) return OXHIP_OK;
    if (h->b_status[query] == OXHIP_ERR_INVALID_START_STATE || h->b_status[query] == OXHIP_ERR_TIMEOUT) {   // no search ran
        for (uint32_t i = 0; i < n; ++i) {
            if (cost) cost[i] = std::numeric_limits<double>::infinity();
            if (hops) hops[i] = 0xFFFFFFFFu;
            if (parent) parent[i] = 0xFFFFFFFFu;
        }
        return OXHIP_OK;
    }
    // the labels are not kept per query: flags, initial labels, label rounds and levels run again for this one (same kernels, and
    // a fixed point that does not depend on the order of arrival: same bits) into workspace row 0
    OX_TRY(select_device(h->cfg.device));
    const PrmBatchArgs b = batch_args(h, query, 1, (uint32_t)(h->bd_res.n / 5));
    const PrmShortestArgs sa = shortest_args(h, h->batch_mode);
    const uint32_t group = prm_batch_group(n, h->n_keys);
    OX_TRY(launch_shortest(h, b, sa, group, false));
    int32_t status = 0;
    HIP_TRY(hipMemcpyAsync(&status, h->bd_res.p, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (cost) HIP_TRY(hipMemcpyAsync(cost, h->bd_label.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (hops) HIP_TRY(hipMemcpyAsync(hops, h->bd_stamp.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    if (parent) HIP_TRY(hipMemcpyAsync(parent, h->bd_parent.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (status == OXHIP_ERR_HIP) return fail(OXHIP_ERR_HIP, "shortest-path search: a label round or level cap was hit, which cannot happen");
    return OXHIP_OK;
}

int32_t oxhip_prm_batch_get_search_stats(oxhip_prm* h, uint32_t* label_rounds, uint64_t* relaxations, double* phase_ms) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (!h->batch_valid) return fail(OXHIP_ERR_UNSAMPLED_STATE_SPACE, "no batch was solved on this roadmap");
    if (h->batch_mode < 0) return fail(OXHIP_ERR_BAD_ARG, "the last batch was not a shortest-path batch");
    const size_t Q = h->b_rounds.size();
    if (label_rounds && Q) std::memcpy(label_rounds, h->b_rounds.data(), Q * sizeof(uint32_t));
    if (relaxations && Q) std::memcpy(relaxations, h->b_relaxed.data(), Q * sizeof(uint64_t));
    if (phase_ms) for (int i = 0; i < 6; ++i) phase_ms[i] = h->short_ms[i];
    return OXHIP_OK;
}

int32_t oxhip_prm_batch_get_results(oxhip_prm* h, int32_t* status, uint32_t* path_len, int32_t* goal_node, uint32_t* n_start, uint32_t* n_goal) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (!h->batch_valid) return fail(OXHIP_ERR_UNSAMPLED_STATE_SPACE, "no batch was solved on this roadmap");
    const size_t Q = h->b_status.size();
    if (status && Q) std::memcpy(status, h->b_status.data(), Q * sizeof(int32_t));
    if (path_len && Q) std::memcpy(path_len, h->b_len.data(), Q * sizeof(uint32_t));
    if (goal_node && Q) std::memcpy(goal_node, h->b_goal_node.data(), Q * sizeof(int32_t));
    if (n_start && Q) std::memcpy(n_start, h->b_nstart.data(), Q * sizeof(uint32_t));
    if (n_goal && Q) std::memcpy(n_goal, h->b_ngoal.data(), Q * sizeof(uint32_t));
    return OXHIP_OK;
}

int32_t oxhip_prm_batch_get_paths(oxhip_prm* h, uint64_t* offsets, uint32_t* nodes, double* states, uint64_t cap_rows, uint64_t* total_rows) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (!h->batch_valid) return fail(OXHIP_ERR_UNSAMPLED_STATE_SPACE, "no batch was solved on this roadmap");
    const uint64_t total = h->b_nodes.size();
    if (total_rows) *total_rows = total;
    if (offsets) std::memcpy(offsets, h->b_off.data(), h->b_off.size() * sizeof(uint64_t));
    if ((nodes || states) && cap_rows < total) return fail(OXHIP_ERR_CAPACITY, "path buffers too small");
    if (nodes && total) std::memcpy(nodes, h->b_nodes.data(), (size_t)total * sizeof(uint32_t));
    if (states && total) std::memcpy(states, h->b_rows.data(), h->b_rows.size() * sizeof(double));
    return OXHIP_OK;
}

int32_t oxhip_prm_batch_get_query_sets(oxhip_prm* h, uint32_t query, uint32_t* start_connections, uint32_t cap_start, uint32_t* n_start,
                                       uint32_t* goal_indices, uint32_t cap_goal, uint32_t* n_goal) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (!h->batch_valid) return fail(OXHIP_ERR_UNSAMPLED_STATE_SPACE, "no batch was solved on this roadmap");
    if (query >= h->b_status.size()) return fail(OXHIP_ERR_BAD_ARG, "query index beyond the last batch");
    const uint32_t ns = h->b_nstart[query], ng = h->b_ngoal[query];
    if (n_start) *n_start = ns;
    if (n_goal) *n_goal = ng;
    if (start_connections && cap_start < ns) return fail(OXHIP_ERR_CAPACITY, "start_connections buffer too small");
    if (goal_indices && cap_goal < ng) return fail(OXHIP_ERR_CAPACITY, "goal_indices buffer too small");
    if ((!start_connections && !goal_indices) || (ns == 0 && ng == 0)) return OXHIP_OK;
    // the sets are not kept per query: the flag kernel runs again for this one (same kernel, same bits) into workspace row 0
    OX_TRY(select_device(h->cfg.device));
    const uint32_t n = h->n;
    const PrmBatchArgs b = batch_args(h, query, 1, (uint32_t)(h->bd_res.n / 5));
    launch_batch_flags(h, b);
    HIP_TRY(hipGetLastError());
    std::vector<uint8_t> flags(n);
    HIP_TRY(hipMemcpyAsync(flags.data(), h->bd_flags.p, n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    uint32_t is = 0, ig = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if ((flags[i] & 1) && start_connections && is < ns) start_connections[is++] = i;
        if ((flags[i] & 2) && goal_indices && ig < ng) goal_indices[ig++] = i;
    }
    return OXHIP_OK;
}

int32_t oxhip_prm_batch_last_timing(oxhip_prm* h, double* phase_ms, uint32_t* rounds) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (phase_ms) for (int i = 0; i < 4; ++i) phase_ms[i] = h->batch_ms[i];
    if (rounds) *rounds = h->batch_rounds;
    return OXHIP_OK;
}

}  // extern "C"

// ---- a roadmap planted from the host, and the roadmap re-checked against the current obstacles

namespace {

// the structure rules of a planted roadmap in the order they are reported (PrmPlantRule)
const char* const kPlantRuleName[kPlantRules] = {
    "offsets_start (offsets[0] must be 0)", "offsets_order (offsets must not decrease)", "neighbour_range (every neighbour < n)",
    "self_loop (no milestone is its own neighbour)", "unsorted (every row strictly ascending)", "asymmetric (v in row u needs u in row v)"};

// the first violated rule among [first, last) of the device's result words, as the refusal
int32_t plant_verdict(oxhip_prm* h, uint32_t* d_viol, uint32_t first, uint32_t last) {
    uint32_t viol[kPlantRules];
    HIP_TRY(hipMemcpyAsync(viol, d_viol, sizeof viol, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (uint32_t r = first; r < last; ++r)
        if (viol[r] != 0xFFFFFFFFu)
            return fail(OXHIP_ERR_BAD_ARG, std::string("roadmap refused: rule ") + kPlantRuleName[r] + ", lowest offending row " + std::to_string(viol[r]));
    return OXHIP_OK;
}

}  // namespace

extern "C" {

int32_t oxhip_prm_set_roadmap(oxhip_prm* h, const double* states, uint32_t n, const uint64_t* offsets, const uint32_t* neighbours) {
    if (!h || !states || !offsets) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    if (!neighbours && offsets[n] != 0) return fail(OXHIP_ERR_BAD_ARG, "null argument: neighbours may be null only when offsets[n] is 0");
    if (!h->is_setup) return fail(OXHIP_ERR_PLANNER_UNINITIALISED, "setup() was not called");
    if (n > h->cfg.max_milestones) return fail(OXHIP_ERR_CAPACITY, "more milestones than max_milestones");
    if (offsets[n] > 0xFFFFFFFFull) return fail(OXHIP_ERR_CAPACITY, "more than 2^32 - 1 directed edge entries");
    const uint32_t dim = h->cfg.dim, n_entries = (uint32_t)offsets[n];
    if (n == 0) {
        if (n_entries) return fail(OXHIP_ERR_BAD_ARG, std::string("roadmap refused: rule ") + kPlantRuleName[kPlantOffsetsStart] + ", lowest offending row 0");
        clear_roadmap(h);   // an empty roadmap: construct_roadmap builds again
        return OXHIP_OK;
    }
    for (size_t k = 0; k < (size_t)n * dim; ++k)   // what set_problem asks of a start (check_query_points)
        if (!(std::fabs(states[k]) <= kMaxMagnitude)) return fail(OXHIP_ERR_BAD_ARG, "milestone coordinate not finite or beyond 1e150");
    OX_TRY(select_device(h->cfg.device));
    // upload and check in staging buffers: a refused call leaves the handle as it was
    DevBuf<double> s_ms;
    DevBuf<uint64_t> s_off64;
    DevBuf<uint32_t> s_off, s_nbrs, s_viol;
    HIP_TRY(s_ms.alloc((size_t)n * dim)); HIP_TRY(s_off64.alloc((size_t)n + 1)); HIP_TRY(s_off.alloc((size_t)n + 1));
    HIP_TRY(s_nbrs.alloc(n_entries)); HIP_TRY(s_viol.alloc(kPlantRules));
    HIP_TRY(hipMemcpyAsync(s_ms.p, states, (size_t)n * dim * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(s_off64.p, offsets, ((size_t)n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    if (n_entries) HIP_TRY(hipMemcpyAsync(s_nbrs.p, neighbours, (size_t)n_entries * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(s_viol.p, 0xFF, kPlantRules * sizeof(uint32_t), h->stream));
    launch_prm_plant_offsets(s_off64.p, n, s_off.p, s_viol.p, h->stream);
    HIP_TRY(hipGetLastError());
    OX_TRY(plant_verdict(h, s_viol.p, kPlantOffsetsStart, kPlantRange));   // the entry rules read rows: only inside proven offsets
    launch_prm_plant_entries(s_off.p, s_nbrs.p, n, n_entries, s_viol.p, h->stream);
    HIP_TRY(hipGetLastError());
    OX_TRY(plant_verdict(h, s_viol.p, kPlantRange, kPlantRules));
    // accepted: the staged roadmap becomes the handle's
    HIP_TRY(hipMemcpyAsync(h->ms.p, s_ms.p, (size_t)n * dim * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->offsets.p, s_off.p, ((size_t)n + 1) * sizeof(uint32_t), hipMemcpyDeviceToDevice, h->stream));
    launch_planted_shadow(h, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    std::swap(h->nbrs.p, s_nbrs.p); std::swap(h->nbrs.n, s_nbrs.n);
    clear_roadmap(h);   // everything that belonged to the roadmap before; n_samples = redraw_batches = 0
    h->n = n;
    h->n_keys = n_entries;
    return OXHIP_OK;
}

int32_t oxhip_prm_revalidate(oxhip_prm* h, uint8_t* milestone_valid, uint32_t* n_invalid_milestones, uint64_t* n_removed_entries) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (!h->is_setup) return fail(OXHIP_ERR_PLANNER_UNINITIALISED, "setup() was not called");
    if (h->n == 0) return fail(OXHIP_ERR_UNSAMPLED_STATE_SPACE, "the roadmap holds no milestones");
    OX_TRY(select_device(h->cfg.device));
    const uint32_t n = h->n, n_old = h->n_keys, pair_cap = n_old / 2 + 1;
    // every buffer before the timed region: hipMalloc is a blocking call
    size_t tmp_bytes = 0;
    HIP_TRY(h->rv_valid.reserve(n)); HIP_TRY(h->rv_counters.reserve(kRevalCounters));
    if (n_old) {
        HIP_TRY(h->rv_keep.reserve(n_old)); HIP_TRY(h->rv_pos.reserve(n_old)); HIP_TRY(h->rv_nbrs.reserve(n_old));
        OX_TRY(reserve_reval_pairs(h, pair_cap));
        HIP_TRY(prm_reval_scan(nullptr, tmp_bytes, h->rv_keep.p, h->rv_pos.p, n_old, h->stream));
        HIP_TRY(h->rv_tmp.reserve(tmp_bytes));
    }
    uint32_t cnt[kRevalCounters] = {};
    HIP_TRY(hipMemsetAsync(h->rv_counters.p, 0, sizeof cnt, h->stream));
    if (n_old) HIP_TRY(hipMemsetAsync(h->rv_keep.p, 0, n_old, h->stream));
    HIP_TRY(hipEventRecord(h->bev[0], h->stream));
    launch_prm_reval_valid(h->so3, h->dp, h->ms.p, n, h->rv_valid.p, h->rv_counters.p, h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->bev[1], h->stream));
    launch_prm_reval_emit(h->offsets.p, h->nbrs.p, h->rv_valid.p, n, n_old, h->rv_pairs.p, reval_cand(h), pair_cap,
                          h->rv_counters.p, h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->bev[2], h->stream));
    HIP_TRY(hipMemcpyAsync(cnt, h->rv_counters.p, sizeof cnt, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (cnt[kRevalPairs] > pair_cap) return fail(OXHIP_ERR_HIP, "revalidate: more lower-index entries than half the roadmap's, which a symmetric roadmap cannot have");
    HIP_TRY(hipEventRecord(h->bev[3], h->stream));
    OX_TRY(launch_reval_edges(h, cnt[kRevalPairs], n, n_old));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->bev[4], h->stream));
    uint32_t n_new = 0;
    if (n_old) {
        HIP_TRY(prm_reval_scan(h->rv_tmp.p, tmp_bytes, h->rv_keep.p, h->rv_pos.p, n_old, h->stream));
        launch_prm_reval_compact(h->offsets.p, h->nbrs.p, h->rv_keep.p, h->rv_pos.p, n, n_old, h->rv_nbrs.p, h->stream);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(h->bev[5], h->stream));
    if (n_old) HIP_TRY(hipMemcpyAsync(&n_new, h->offsets.p + n, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    if (milestone_valid) HIP_TRY(hipMemcpyAsync(milestone_valid, h->rv_valid.p, n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (n_old) { std::swap(h->nbrs.p, h->rv_nbrs.p); std::swap(h->nbrs.n, h->rv_nbrs.n); }
    h->reval_ms[0] = elapsed_ms(h->bev[0], h->bev[1]);
    h->reval_ms[1] = elapsed_ms(h->bev[1], h->bev[2]);
    h->reval_ms[2] = elapsed_ms(h->bev[3], h->bev[4]);
    h->reval_ms[3] = elapsed_ms(h->bev[4], h->bev[5]);
    h->n_keys = n_new;
    drop_derived(h);   // the host copy (the single solve searches it), the last solve's sets, the last batch, the edge weights
    if (n_invalid_milestones) *n_invalid_milestones = cnt[kRevalInvalid];
    if (n_removed_entries) *n_removed_entries = (uint64_t)n_old - n_new;
    return OXHIP_OK;
}

int32_t oxhip_prm_revalidate_last_timing(oxhip_prm* h, double* phase_ms) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (phase_ms) for (int i = 0; i < 4; ++i) phase_ms[i] = h->reval_ms[i];
    return OXHIP_OK;
}

}  // extern "C"

// ---- a roadmap grown in place: oxhip_prm_grow_roadmap in its steps

namespace {

// which earlier milestones are live: is_valid(milestone i) now, by the re-check's own kernel, into rv_valid; n_dead = its zeros
int32_t liveness_mask(oxhip_prm* h, uint32_t& n_dead) {
    uint32_t cnt[kRevalCounters] = {};
    HIP_TRY(h->rv_valid.reserve(h->n)); HIP_TRY(h->rv_counters.reserve(kRevalCounters));
    HIP_TRY(hipMemsetAsync(h->rv_counters.p, 0, sizeof cnt, h->stream));
    HIP_TRY(hipEventRecord(h->ev[0], h->stream));
    launch_prm_reval_valid(h->so3, h->dp, h->ms.p, h->n, h->rv_valid.p, h->rv_counters.p, h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev[1], h->stream));
    HIP_TRY(hipMemcpyAsync(cnt, h->rv_counters.p, sizeof cnt, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->grow_ms[0] = elapsed_ms(h->ev[0], h->ev[1]);
    n_dead = cnt[kRevalInvalid];
    return OXHIP_OK;
}

// every buffer alloc_prm sizes by the capacity, moved to `cap` with the roadmap's part of its contents (the query flags hold
// nothing between calls)
int32_t grow_capacity(oxhip_prm* h, uint32_t cap) {
    const size_t dim = h->cfg.dim, n = h->n;
    DevBuf<double> ms;
    DevBuf<float> ms32;
    DevBuf<uint8_t> flags;
    DevBuf<uint32_t> offsets;
    HIP_TRY(ms.alloc(dim * cap)); HIP_TRY(flags.alloc(cap)); HIP_TRY(offsets.alloc((size_t)cap + 1));
    if (!h->so3) HIP_TRY(ms32.alloc(dim * cap));
    HIP_TRY(hipMemcpyAsync(ms.p, h->ms.p, n * dim * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    if (!h->so3) HIP_TRY(hipMemcpyAsync(ms32.p, h->ms32.p, n * dim * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(offsets.p, h->offsets.p, (n + 1) * sizeof(uint32_t), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    std::swap(ms.p, h->ms.p); std::swap(ms.n, h->ms.n);
    std::swap(ms32.p, h->ms32.p); std::swap(ms32.n, h->ms32.n);
    std::swap(flags.p, h->flags.p); std::swap(flags.n, h->flags.n);
    std::swap(offsets.p, h->offsets.p); std::swap(offsets.n, h->offsets.n);
    h->args.ms = h->ms.p; h->args.ms32 = h->ms32.p; h->args.cap = cap;
    return OXHIP_OK;
}

// the directed keys of the roadmap as it stands, under the current capacity's shift: what this call's edge keys are appended to
int32_t keys_from_csr(oxhip_prm* h) {
    HIP_TRY(h->keys.reserve(std::max<size_t>(h->n_keys, 1)));
    h->args.keys = h->keys.p;
    HIP_TRY(hipEventRecord(h->ev[0], h->stream));
    launch_prm_grow_keys(h->offsets.p, h->nbrs.p, h->n, h->n_keys, prm_key_shift(h->args.cap), h->keys.p, h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev[1], h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->grow_ms[1] = elapsed_ms(h->ev[0], h->ev[1]);
    return OXHIP_OK;
}

// the candidates whose earlier end is live, into gw_cand: `pairs` and st.n_cand come back as what the edge step reads
int32_t drop_dead_candidates(oxhip_prm* h, PrmState& st, uint32_t n_old, uint2*& pairs) {
    const uint32_t nc = (uint32_t)st.n_cand;
    uint32_t kept = 0;
    HIP_TRY(h->gw_cand.reserve(std::max<uint32_t>(nc, 1))); HIP_TRY(h->gw_count.reserve(1));
    HIP_TRY(hipMemsetAsync(h->gw_count.p, 0, sizeof(uint32_t), h->stream));
    HIP_TRY(hipEventRecord(h->ev[2], h->stream));
    launch_prm_grow_filter(pairs, nc, h->rv_valid.p, n_old, h->gw_cand.p, h->gw_count.p, h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev[3], h->stream));
    HIP_TRY(hipMemcpyAsync(&kept, h->gw_count.p, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->t_ms[1] += elapsed_ms(h->ev[2], h->ev[3]);
    st.n_cand = kept;
    pairs = h->gw_cand.p;
    return OXHIP_OK;
}

// construction's round for the milestones [n_old, n_now) on the roadmap that exists: sample, pairs, edges, sort + CSR
int32_t grow_round(oxhip_prm* h, PrmState& st, uint32_t n_more, uint64_t sample_limit, bool any_dead) {
    const uint32_t n_old = h->n, knn_k = h->cfg.knn_k;
    OX_TRY(write_state(h, st));
    HIP_TRY(hipEventRecord(h->ev[0], h->stream));
    OX_TRY(sample_until(h, st, n_old + n_more, sample_limit));
    HIP_TRY(hipEventRecord(h->ev[1], h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->t_ms[0] = elapsed_ms(h->ev[0], h->ev[1]);
    const uint32_t n_now = st.n_milestones;
    if (n_now > n_old && n_now >= 2 && (h->thr_conn >= 0.0 || knn_k)) {   // (construct_roadmap's condition)
        if (knn_k) OX_TRY(knn_row_radii(h, st, n_old, n_now));
        OX_TRY(find_pairs(h, st, n_old, n_now));
        uint2* pairs = h->cand.p;
        if (knn_k) OX_TRY(knn_select(h, st, n_old, n_now, pairs));
        else if (any_dead) OX_TRY(drop_dead_candidates(h, st, n_old, pairs));   // no dead milestone: exactly construction's candidates
        OX_TRY(reserve_keys(h, st));
        OX_TRY(check_edges(h, st, pairs));
    }
    return build_csr(h, n_now, st.n_keys);
}

}  // namespace

extern "C" {

int32_t oxhip_prm_grow_roadmap(oxhip_prm* h, const oxhip_prm_grow_config* g, uint32_t* n_added, uint64_t* n_samples_drawn) {
    if (!h || !g || !n_added || !n_samples_drawn) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    if (g->struct_size != sizeof(oxhip_prm_grow_config)) return fail(OXHIP_ERR_BAD_ARG, "struct_size mismatch");
    *n_added = 0;
    *n_samples_drawn = 0;
    if (g->n_more == 0) return fail(OXHIP_ERR_BAD_ARG, "n_more must be at least 1");
    if (g->flags & ~OXHIP_PRM_GROW_NEW_STREAM) return fail(OXHIP_ERR_BAD_ARG, "unknown flag (OXHIP_PRM_GROW_NEW_STREAM is the only one)");
    if (!h->is_setup) return fail(OXHIP_ERR_PLANNER_UNINITIALISED, "setup() was not called");
    if (h->n == 0) return fail(OXHIP_ERR_UNSAMPLED_STATE_SPACE, "the roadmap holds no milestones: construct_roadmap() builds one");
    const bool new_stream = (g->flags & OXHIP_PRM_GROW_NEW_STREAM) != 0;
    if (!new_stream && !h->pos_valid)
        return fail(OXHIP_ERR_BAD_ARG, "this roadmap was not constructed by this handle, so there is no stream position to continue: "
                                       "pass OXHIP_PRM_GROW_NEW_STREAM with a stream id");
    const uint32_t n_old = h->n;
    if ((uint64_t)n_old + g->n_more > (1ull << 26)) return fail(OXHIP_ERR_CAPACITY, "n + n_more exceeds 2^26 milestones");
    OX_TRY(select_device(h->cfg.device));
    uint32_t n_dead = 0;
    OX_TRY(liveness_mask(h, n_dead));
    if (h->cfg.knn_k && n_dead)
        return fail(OXHIP_ERR_BAD_ARG, "k-nearest growth over invalid milestones is not built (" + std::to_string(n_dead) + " are invalid now)");
    if (n_old + g->n_more > h->args.cap) {
        uint32_t cap = 1024;   // the next power of two: above alloc_prm's multiple of 1024, at most 2^26
        while (cap < n_old + g->n_more) cap *= 2;
        OX_TRY(grow_capacity(h, cap));
    }
    OX_TRY(keys_from_csr(h));
    // construction's phase times are its own: this call's go to grow_ms
    double construct_ms[6];
    std::memcpy(construct_ms, h->t_ms, sizeof construct_ms);
    for (double& t : h->t_ms) t = 0.0;
    const uint64_t budget = g->max_samples ? g->max_samples : 4096ull * g->n_more + (1ull << 22);
    const uint64_t sample_limit = budget > ~0ull - h->n_samples ? ~0ull : h->n_samples + budget;
    PrmState st{};
    st.draws = new_stream ? 0 : h->pos_draws;
    st.n_samples = h->n_samples;
    st.n_milestones = n_old;
    st.n_keys = h->n_keys;
    st.redraw_batches = h->redraw_batches;
    h->args.stream = new_stream ? g->stream : h->pos_stream;
    const int32_t status = grow_round(h, st, g->n_more, sample_limit, n_dead != 0);
    const uint64_t stream_used = h->args.stream;
    h->args.stream = h->cfg.stream;   // construct_roadmap after a setup() draws from the configured stream
    for (int i = 0; i < 4; ++i) h->grow_ms[2 + i] = h->t_ms[i];
    std::memcpy(h->t_ms, construct_ms, sizeof construct_ms);
    if (status != OXHIP_OK) return status;
    *n_added = st.n_milestones - n_old;
    *n_samples_drawn = st.n_samples - h->n_samples;
    h->n = st.n_milestones;
    h->n_keys = st.n_keys;
    h->n_samples = st.n_samples;
    h->redraw_batches = st.redraw_batches;
    h->pos_valid = true; h->pos_stream = stream_used; h->pos_draws = st.draws;
    drop_derived(h);   // the host copy, the last solve's sets, the last batch, the edge weights
    return OXHIP_OK;
}

int32_t oxhip_prm_grow_last_timing(oxhip_prm* h, double* phase_ms) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (phase_ms) for (int i = 0; i < 6; ++i) phase_ms[i] = h->grow_ms[i];
    return OXHIP_OK;
}

}  // extern "C"

// ---- the roadmap as a graph: its connected components, and the roadmap pruned

namespace {

PrmCcBuffers cc_buffers(oxhip_prm* h) { return PrmCcBuffers{h->cc_parent.p, h->cc_label.p, h->cc_count.p, h->cc_size.p, h->cc_summary.p}; }

// the union-find's arrays for the roadmap as it stands: before any timed region (hipMalloc is a blocking call)
int32_t reserve_components(oxhip_prm* h) {
    const size_t n = h->n;
    HIP_TRY(h->cc_parent.reserve(n)); HIP_TRY(h->cc_label.reserve(n)); HIP_TRY(h->cc_count.reserve(n)); HIP_TRY(h->cc_size.reserve(n));
    HIP_TRY(h->cc_summary.reserve(kCcSummaryWords));
    return OXHIP_OK;
}

// labels, sizes and summary of the CSR into the cc_ buffers; alive (device, [n], or null): prune's stage-1 survivors.  Records
// the events first .. first + 3 around its three phases; the kept labels are the whole roadmap's only without a mask.
int32_t components_of(oxhip_prm* h, const uint8_t* alive, uint32_t first) {
    h->cc_valid = false;
    HIP_TRY(hipEventRecord(h->cev[first], h->stream));
    launch_prm_components(h->offsets.p, h->nbrs.p, alive, h->n, h->n_keys, cc_buffers(h), h->cev[first + 1], h->cev[first + 2], h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->cev[first + 3], h->stream));
    return OXHIP_OK;
}

// every refusal of oxhip_prm_prune that needs neither the handle's contents nor a device
int32_t validate_prune_args(const oxhip_prm* h, const oxhip_prm_prune_config* c, const uint8_t* keep) {
    constexpr uint32_t known = OXHIP_PRM_PRUNE_INVALID | OXHIP_PRM_PRUNE_MASK | OXHIP_PRM_PRUNE_MIN_SIZE | OXHIP_PRM_PRUNE_LARGEST;
    if (!h || !c) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    if (c->struct_size != sizeof(oxhip_prm_prune_config)) return fail(OXHIP_ERR_BAD_ARG, "struct_size mismatch");
    if (c->flags == 0) return fail(OXHIP_ERR_BAD_ARG, "flags must name at least one of OXHIP_PRM_PRUNE_INVALID, _MASK, _MIN_SIZE, _LARGEST");
    if (c->flags & ~known) return fail(OXHIP_ERR_BAD_ARG, "unknown flag (OXHIP_PRM_PRUNE_INVALID, _MASK, _MIN_SIZE and _LARGEST are the four)");
    if (c->pad != 0) return fail(OXHIP_ERR_BAD_ARG, "pad must be 0");
    if ((c->flags & OXHIP_PRM_PRUNE_MASK) && !keep) return fail(OXHIP_ERR_BAD_ARG, "OXHIP_PRM_PRUNE_MASK needs a keep mask");
    if (!(c->flags & OXHIP_PRM_PRUNE_MASK) && keep) return fail(OXHIP_ERR_BAD_ARG, "a keep mask needs OXHIP_PRM_PRUNE_MASK");
    if ((c->flags & OXHIP_PRM_PRUNE_MIN_SIZE) && c->min_size == 0) return fail(OXHIP_ERR_BAD_ARG, "OXHIP_PRM_PRUNE_MIN_SIZE needs min_size >= 1");
    return OXHIP_OK;
}

// every buffer of a prune before its timed region: masks, scans, the second buffers the compaction writes
int32_t reserve_prune(oxhip_prm* h, uint32_t flags, size_t& tmp_bytes) {
    const size_t n = h->n, ne = h->n_keys, dim = h->cfg.dim, cap = h->args.cap;
    HIP_TRY(h->pr_keep.reserve(n)); HIP_TRY(h->pr_pos.reserve(n)); HIP_TRY(h->pr_index.reserve(n)); HIP_TRY(h->pr_kept.reserve(2));
    if (flags & OXHIP_PRM_PRUNE_MASK) HIP_TRY(h->pr_mask.reserve(n));
    if (flags & OXHIP_PRM_PRUNE_INVALID) { HIP_TRY(h->rv_valid.reserve(n)); HIP_TRY(h->rv_counters.reserve(kRevalCounters)); }
    if (flags & (OXHIP_PRM_PRUNE_MIN_SIZE | OXHIP_PRM_PRUNE_LARGEST)) OX_TRY(reserve_components(h));
    HIP_TRY(h->pr_ekeep.reserve(std::max<size_t>(ne, 1))); HIP_TRY(h->pr_epos.reserve(std::max<size_t>(ne, 1)));
    HIP_TRY(h->pr_nbrs.reserve(std::max<size_t>(ne, 1)));
    if (h->pr_offsets.n != cap + 1) HIP_TRY(h->pr_offsets.alloc(cap + 1));   // swapped with offsets: the capacity's size exactly
    if (h->pr_ms.n != dim * cap) HIP_TRY(h->pr_ms.alloc(dim * cap));
    if (!h->so3 && h->pr_ms32.n != dim * cap) HIP_TRY(h->pr_ms32.alloc(dim * cap));
    size_t a = 0, b = 0;
    HIP_TRY(prm_reval_scan(nullptr, a, h->pr_keep.p, h->pr_pos.p, (uint32_t)n, h->stream));
    if (ne) HIP_TRY(prm_reval_scan(nullptr, b, h->pr_ekeep.p, h->pr_epos.p, (uint32_t)ne, h->stream));
    tmp_bytes = std::max(a, b);
    HIP_TRY(h->rv_tmp.reserve(tmp_bytes));
    return OXHIP_OK;
}

// stage 1 into pr_keep: INVALID by the re-check's own milestone kernel (as liveness_mask), MASK from the caller's bytes (pr_mask)
int32_t prune_stage1_mask(oxhip_prm* h, uint32_t flags) {
    const uint8_t *valid = nullptr, *mask = nullptr;
    if (flags & OXHIP_PRM_PRUNE_INVALID) {
        HIP_TRY(hipMemsetAsync(h->rv_counters.p, 0, kRevalCounters * sizeof(uint32_t), h->stream));
        launch_prm_reval_valid(h->so3, h->dp, h->ms.p, h->n, h->rv_valid.p, h->rv_counters.p, h->stream);
        HIP_TRY(hipGetLastError());
        valid = h->rv_valid.p;
    }
    if (flags & OXHIP_PRM_PRUNE_MASK) mask = h->pr_mask.p;
    launch_prm_prune_stage1(valid, mask, h->n, h->pr_keep.p, h->pr_kept.p, h->stream);
    HIP_TRY(hipGetLastError());
    return OXHIP_OK;
}

// stage 2 on the components of the stage-1 survivors (cc_ buffers): MIN_SIZE and LARGEST into pr_keep
int32_t prune_stage2_mask(oxhip_prm* h, const oxhip_prm_prune_config* c) {
    launch_prm_prune_stage2(cc_buffers(h), h->n, (c->flags & OXHIP_PRM_PRUNE_MIN_SIZE) ? c->min_size : 0u,
                            (c->flags & OXHIP_PRM_PRUNE_LARGEST) != 0, h->pr_keep.p, h->pr_kept.p + 1, h->stream);
    HIP_TRY(hipGetLastError());
    return OXHIP_OK;
}

// the roadmap of the n_kept milestones of pr_keep, into the second buffers; the handle takes them when everything has run
int32_t compact_roadmap(oxhip_prm* h, uint32_t n_kept, size_t tmp_bytes, int32_t* new_index, uint32_t& n_entries_new) {
    const uint32_t n = h->n, ne = h->n_keys, dim = h->cfg.dim;
    HIP_TRY(hipEventRecord(h->cev[6], h->stream));
    HIP_TRY(prm_reval_scan(h->rv_tmp.p, tmp_bytes, h->pr_keep.p, h->pr_pos.p, n, h->stream));
    launch_prm_prune_flags(h->offsets.p, h->nbrs.p, h->pr_keep.p, h->pr_pos.p, n, ne, h->pr_index.p, h->pr_ekeep.p, h->stream);
    HIP_TRY(hipGetLastError());
    if (ne) HIP_TRY(prm_reval_scan(h->rv_tmp.p, tmp_bytes, h->pr_ekeep.p, h->pr_epos.p, ne, h->stream));
    HIP_TRY(hipEventRecord(h->cev[7], h->stream));
    if (ne) launch_prm_prune_entries(h->offsets.p, h->nbrs.p, h->pr_ekeep.p, h->pr_epos.p, h->pr_index.p, n, ne, n_kept, h->pr_offsets.p,
                                     h->pr_nbrs.p, h->stream);
    else HIP_TRY(hipMemsetAsync(h->pr_offsets.p, 0, ((size_t)n_kept + 1) * sizeof(uint32_t), h->stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->cev[8], h->stream));
    launch_prm_prune_states(h->ms.p, h->so3 ? nullptr : h->ms32.p, h->pr_index.p, n, dim, h->pr_ms.p, h->so3 ? nullptr : h->pr_ms32.p, h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->cev[9], h->stream));
    n_entries_new = 0;
    if (ne) HIP_TRY(hipMemcpyAsync(&n_entries_new, h->pr_offsets.p + n_kept, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    if (new_index) HIP_TRY(hipMemcpyAsync(new_index, h->pr_index.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    std::swap(h->offsets.p, h->pr_offsets.p); std::swap(h->offsets.n, h->pr_offsets.n);
    std::swap(h->nbrs.p, h->pr_nbrs.p); std::swap(h->nbrs.n, h->pr_nbrs.n);
    std::swap(h->ms.p, h->pr_ms.p); std::swap(h->ms.n, h->pr_ms.n);
    if (!h->so3) { std::swap(h->ms32.p, h->pr_ms32.p); std::swap(h->ms32.n, h->pr_ms32.n); }
    h->args.ms = h->ms.p; h->args.ms32 = h->ms32.p;
    return OXHIP_OK;
}

}  // namespace

extern "C" {

int32_t oxhip_prm_components(oxhip_prm* h, uint32_t* label, uint32_t* size, uint32_t cap, uint32_t* n_components, uint32_t* largest_label,
                             uint32_t* largest_size) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (!h->is_setup) return fail(OXHIP_ERR_PLANNER_UNINITIALISED, "setup() was not called");
    if (h->n == 0) return fail(OXHIP_ERR_UNSAMPLED_STATE_SPACE, "the roadmap holds no milestones");
    if ((label || size) && cap < h->n) return fail(OXHIP_ERR_CAPACITY, "label / size buffers too small");
    OX_TRY(select_device(h->cfg.device));
    const uint32_t n = h->n;
    const bool compute = !h->cc_valid;
    if (compute) {
        OX_TRY(reserve_components(h));
        OX_TRY(components_of(h, nullptr, 0));
    }
    unsigned long long summary[kCcSummaryWords] = {};
    HIP_TRY(hipEventRecord(h->cev[4], h->stream));
    HIP_TRY(hipMemcpyAsync(summary, h->cc_summary.p, sizeof summary, hipMemcpyDeviceToHost, h->stream));
    if (label) HIP_TRY(hipMemcpyAsync(label, h->cc_label.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    if (size) HIP_TRY(hipMemcpyAsync(size, h->cc_size.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipEventRecord(h->cev[5], h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->cc_ms[0] = compute ? elapsed_ms(h->cev[0], h->cev[1]) : 0.0;
    h->cc_ms[1] = compute ? elapsed_ms(h->cev[1], h->cev[2]) : 0.0;
    h->cc_ms[2] = compute ? elapsed_ms(h->cev[2], h->cev[3]) : 0.0;
    h->cc_ms[3] = elapsed_ms(h->cev[4], h->cev[5]);
    h->cc_valid = true;
    if (n_components) *n_components = (uint32_t)summary[kCcRoots];
    if (largest_label) *largest_label = 0xFFFFFFFFu - (uint32_t)summary[kCcBest];
    if (largest_size) *largest_size = (uint32_t)(summary[kCcBest] >> 32);
    return OXHIP_OK;
}

int32_t oxhip_prm_components_last_timing(oxhip_prm* h, double* phase_ms, uint32_t* launches) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (phase_ms) for (int i = 0; i < 4; ++i) phase_ms[i] = h->cc_ms[i];
    if (launches) *launches = kCcLaunches;
    return OXHIP_OK;
}

int32_t oxhip_prm_prune(oxhip_prm* h, const oxhip_prm_prune_config* c, const uint8_t* keep, int32_t* new_index, uint32_t* n_kept,
                        uint64_t* n_removed_entries) {
    OX_TRY(validate_prune_args(h, c, keep));
    if (!h->is_setup) return fail(OXHIP_ERR_PLANNER_UNINITIALISED, "setup() was not called");
    if (h->n == 0) return fail(OXHIP_ERR_UNSAMPLED_STATE_SPACE, "the roadmap holds no milestones");
    OX_TRY(select_device(h->cfg.device));
    const uint32_t n = h->n, n_old = h->n_keys;
    const bool stage2 = (c->flags & (OXHIP_PRM_PRUNE_MIN_SIZE | OXHIP_PRM_PRUNE_LARGEST)) != 0;
    size_t tmp_bytes = 0;
    OX_TRY(reserve_prune(h, c->flags, tmp_bytes));
    if (c->flags & OXHIP_PRM_PRUNE_MASK) HIP_TRY(hipMemcpyAsync(h->pr_mask.p, keep, n, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(h->pr_kept.p, 0, 2 * sizeof(uint32_t), h->stream));
    HIP_TRY(hipEventRecord(h->cev[4], h->stream));
    OX_TRY(prune_stage1_mask(h, c->flags));
    if (stage2) {   // (the labels of the stage-1 survivors are not the roadmap's: components_of forgets the kept ones)
        OX_TRY(components_of(h, h->pr_keep.p, 0));
        OX_TRY(prune_stage2_mask(h, c));
    }
    HIP_TRY(hipEventRecord(h->cev[5], h->stream));
    uint32_t kept[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(kept, h->pr_kept.p, sizeof kept, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const uint32_t n_new = stage2 ? kept[1] : kept[0];
    if (n_new == 0) return fail(OXHIP_ERR_BAD_ARG, "would keep no milestone");   // only workspace was written so far
    uint32_t n_entries_new = 0;
    OX_TRY(compact_roadmap(h, n_new, tmp_bytes, new_index, n_entries_new));
    // masks = stage 1 and stage 2 around the components; components = the union-find's three phases
    const double comp = stage2 ? elapsed_ms(h->cev[0], h->cev[3]) : 0.0;
    h->prune_ms[0] = stage2 ? elapsed_ms(h->cev[4], h->cev[0]) + elapsed_ms(h->cev[3], h->cev[5]) : elapsed_ms(h->cev[4], h->cev[5]);
    h->prune_ms[1] = comp;
    h->prune_ms[2] = elapsed_ms(h->cev[6], h->cev[7]);
    h->prune_ms[3] = elapsed_ms(h->cev[7], h->cev[8]);
    h->prune_ms[4] = elapsed_ms(h->cev[8], h->cev[9]);
    h->n = n_new;
    h->n_keys = n_entries_new;
    drop_derived(h);   // the host copy, the last solve's sets, the last batch, the edge weights, the kept component labels
    if (n_kept) *n_kept = n_new;
    if (n_removed_entries) *n_removed_entries = (uint64_t)n_old - n_entries_new;
    return OXHIP_OK;
}

int32_t oxhip_prm_prune_last_timing(oxhip_prm* h, double* phase_ms) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (phase_ms) for (int i = 0; i < 5; ++i) phase_ms[i] = h->prune_ms[i];
    return OXHIP_OK;
}

}  // extern "C"
