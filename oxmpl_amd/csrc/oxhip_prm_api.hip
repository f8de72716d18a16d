// oxhip_prm_api.hip -- the PRM part of the C ABI (include/oxmpl_hip.h, oxhip_prm_*).
//
// Host side of oxmpl's PRM (oxmpl/src/geometric/planners/prm.rs): owns the device roadmap and drives the kernels of prm_kernels.hip
// (space = OXHIP_SPACE_SO3: prm_so3.hip).  No CPU fallback: without a HIP device every computing entry point fails.
// The handle (struct oxhip_prm) holds the roadmap as one value (PrmRoadmap) and one member per service -- sampler, k-nearest,
// construction's workspace and tally, single query, batch, shortest, re-check, growth, components, prune, simplify -- each with its clock
// (PhaseClock, oxhip_host.hpp), phase times and validity flag.  Each entry point is a sequence of named steps (DESIGN.md section 1,
// "PRM host side"): create = validate_prm_config, select_device, fill_prm_params, alloc_prm; construct_roadmap = the reference's loop
// over sample_until, knn_row_radii, find_pairs, knn_select, reserve_keys, check_edges, then build_csr, adding up into the tally their
// caller gives them; solve = query_sets, prm_bfs_path (oxhip_host.hpp, on the CSR roadmap copied back once per roadmap), the path;
// solve_batch[_shortest] (sections 17, 19) = stage_batch, reserve_batch_workspace, then per round run_round, scatter_round,
// extract_round_paths; revalidate (section 20) and the two below start from milestone_validity; grow_roadmap (section 23) = that
// liveness mask, grow_capacity, keys_from_csr, then grow_round: construction's steps into growth's tally, with drop_dead_candidates
// before the edges; components (section 24) = components_of, then the copies; prune = prune_stage1_mask, components_of(alive),
// prune_stage2_mask, compact_roadmap; batch_simplify_paths (section 25) = reserve_simplify_workspace, stage_paths, then per round
// subdivide_round, pairs_round, dp_round, collect_round (the workspace is reserved before the paths are staged, not after as the
// steps were first listed: the reservation is where a path too large is refused, and a refused call keeps the last results).  The space is named by the dispatchers below the handle, the per-space part of the sampler,
// the steps of create, the two obstacle setters and the prm_shortest launches that take it as an argument.
#include <algorithm>
#include <chrono>
#include <cstring>

#include "oxhip_host.hpp"
#include "oxhip_internal.hpp"
#include "rrt_device.hpp"

using namespace oxhip;

// The roadmap as one value: what replaces one of its buffers ends in bind_roadmap, what changes it in drop_derived / clear_roadmap.
struct PrmBuffers {
    DevBuf<double> ms;                // milestones, [dim][capacity]
    DevBuf<float> ms32;               // their fl32 shadow (the R^n pair-search screen; SO(3) has none)
    DevBuf<uint32_t> offsets, nbrs;   // CSR: [capacity + 1], [n_keys]
};
struct PrmRoadmap : PrmBuffers {
    uint32_t n = 0, n_keys = 0;       // milestones, directed edge entries
};

// What the steps of a construction or of a growth add up, given to them by their caller, with the clock they time themselves by:
// each step brackets itself (kBegin, kEnd) and reads the clock before the next one starts.
enum Span { kBegin, kEnd };
struct PrmBuildTally {
    PhaseClock clk{2};
    double ms[4] = {};          // sample, pairs (+ k-nearest selection, + growth's filter), edges, sort + CSR
    uint64_t candidates = 0;    // in-radius pairs found
    uint32_t exact_rows = 0;    // k-nearest rows that needed the exact search
    void reset() { for (double& t : ms) t = 0.0; candidates = 0; exact_rows = 0; }
};

// the other clocks' marks (kLabelsEnd: shortest paths only; kCcBegin .. kCcEnd and kPrCcBegin .. kPrCcEnd: components_of's four)
enum BatchMark { kRoundBegin, kFlagsEnd, kLabelsEnd, kSearchEnd, kResultsEnd, kPathsBegin, kPathsEnd, kRowsEnd };
enum RevalMark { kRvBegin, kRvValidEnd, kRvEmitEnd, kRvEdgesBegin, kRvEdgesEnd, kRvCompactEnd };
enum CcMark { kCcBegin, kCcHooked, kCcFlat, kCcEnd, kCcCopyBegin, kCcCopyEnd };
enum PruneMark { kPrBegin, kPrCcBegin, kPrCcEnd = kPrCcBegin + 3, kPrMasksEnd, kPrScanBegin, kPrScanEnd, kPrEntriesEnd, kPrStatesEnd };

// The handle: the configuration, the roadmap, and per service its workspace, clock, last call's phase times (ms) and validity flag.
struct oxhip_prm {
    oxhip_prm_config cfg{};
    DevParams dp{};           // space, resolution and validity field (the RRT fields stay zero)
    PrmArgs args{};
    double thr_conn = -1.0;   // d2 <= thr_conn  <=>  distance < connection_radius
    bool so3 = false;         // OXHIP_SPACE_SO3: quaternion milestones, cones, prm_so3.hip
    double so3_lo = -1.0, so3_hi = -1.0;   // |dot| bands of the SO(3) radius test (so3_radius_bands)
    double maxabs = 1.0;      // largest |coordinate| of bounds and sphere centres (midpoint filter margin)
    bool is_setup = false;
    hipStream_t stream = nullptr;
    struct { DevBuf<double> sph_c, sph_thr, sph_r, box_lo, box_hi; } obs;
    PrmRoadmap rm;
    PrmBuffers spare;   // the second buffers a prune compacts into, swapped with rm's buffer by buffer
    struct {   // parallel sampler scratch (one round), and where the roadmap's samples came from
        DevBuf<double> tmp;
        DevBuf<uint64_t> vbits;
        DevBuf<uint32_t> off, flag;
        DevBuf<uint64_t> abits;    // SO(3) sampler: accepted-attempt ballots and counts
        DevBuf<uint32_t> acnt;
        double valid_rate = 1.0;   // running estimate of P(sample is valid), sizes the rounds
        uint64_t n_samples = 0;
        uint32_t redraw_batches = 0;
        // where the sampler stopped (stream id, u64 word), for oxhip_prm_grow_roadmap: set by construct_roadmap / grow_roadmap,
        // forgotten by setup / set_roadmap
        bool pos_valid = false;
        uint64_t pos_stream = 0, pos_draws = 0;
    } sampler;
    struct {   // k-nearest variant: per-row candidate radii, the sorted candidates and their distances, the selected pairs
        DevBuf<double> thr, dist;
        DevBuf<float> thr32;
        DevBuf<uint64_t> keys, sorted;
        DevBuf<uint2> sel;
        DevBuf<uint32_t> counters, failed;
    } knn;
    struct {   // construction's device state, candidate pairs, directed keys and their sort
        DevBuf<PrmState> state;
        DevBuf<uint2> cand;
        DevBuf<uint64_t> keys, keys_sorted;
        DevBuf<uint8_t> sort_tmp;
    } work;
    PrmBuildTally built;   // the last construct_roadmap (its two counters: plus every grow since, see oxhip_prm_grow_roadmap)
    struct {   // the single query (oxhip_prm_solve): the host copy of the roadmap it searches, the last query and its sets
        PhaseClock clk{2};
        double ms[2] = {};         // query kernel, bfs (host); zeroed by construct_roadmap with its own four
        bool host_copy = false;    // h_offsets / h_nbrs / h_states are current
        std::vector<uint32_t> h_offsets, h_nbrs;
        std::vector<double> h_states;  // AoS [n][dim]
        PrmQuery query{};
        DevBuf<uint8_t> flags;     // [capacity]
        DevBuf<uint32_t> start_valid;
        std::vector<uint32_t> start_conn, goal_idx;
    } single;
    struct {   // the last oxhip_prm_solve_batch[_shortest]: its queries, per-query results and all paths
        PhaseClock clk{8};
        double ms[4] = {};   // flag kernels, search kernels, path extraction, device-to-host copies
        bool valid = false;
        uint32_t rounds = 0;
        int32_t mode = -1;   // weights mode of the last batch, -1: it was the breadth-first oxhip_prm_solve_batch
        std::vector<double> starts, goals, thr, filt;   // as uploaded: [Q][dim], [Q][dim], [Q], [Q]
        std::vector<int32_t> status, goal_node;
        std::vector<uint32_t> len, nstart, ngoal, nodes;
        std::vector<uint64_t> off;                      // [Q + 1] row offsets of the paths
        std::vector<double> rows;
        // d_: the per-round device workspace
        DevBuf<double> d_starts, d_goals, d_thr, d_filt, d_rows;
        DevBuf<uint8_t> d_flags;
        DevBuf<uint32_t> d_start_valid, d_parent, d_queue, d_res, d_nodes;
        DevBuf<uint64_t> d_off;
    } batch;
    struct {   // oxhip_prm_solve_batch_shortest: the edge weights live until the roadmap changes; the rest is the last batch's
        PhaseClock clk{2};   // the edge weights' bracket (a round is timed by the batch's clock)
        double ms[6] = {};   // edge weights (when this batch computed them), flags + initial labels, label rounds, tight levels, paths, copies
        bool w_valid = false;      // w_edges holds the distances of the roadmap's CSR entries
        DevBuf<double> w_edges;
        std::vector<double> cost;
        std::vector<uint32_t> rounds;
        std::vector<uint64_t> relaxed;
        DevBuf<uint64_t> d_label;
        DevBuf<uint32_t> d_stamp, d_rounds;
        DevBuf<double> d_cost;
        DevBuf<unsigned long long> d_relaxed;
    } shortest;
    struct {   // oxhip_prm_revalidate: its workspace and the phase times of the last call
        PhaseClock clk{6};
        double ms[4] = {};   // milestone validity, pair emission, edge checks, compaction
        DevBuf<uint8_t> valid, keep, tmp;   // (valid, counters: milestone_validity's, so growth's and prune's too; tmp: prune's scans too)
        DevBuf<uint32_t> pos, counters;
        DevBuf<uint32_t> nbrs;       // the second neighbour buffer the compaction writes, swapped with rm.nbrs
        DevBuf<uint4> pairs;
        DevBuf<uint2> cand;          // SO(3): the pairs as construction's edge kernel reads them, the keys it emits and their count
        DevBuf<uint64_t> keys;
        DevBuf<PrmState> state;
    } reval;
    struct {   // oxhip_prm_grow_roadmap: what the last call's steps added up, the filtered candidates
        PrmBuildTally tally;
        double mask_ms = 0.0, keys_ms = 0.0;   // liveness mask, keys from CSR (timed by the tally's clock, before its steps)
        DevBuf<uint2> cand;
        DevBuf<uint32_t> count;
    } grow;
    struct {   // oxhip_prm_components: the union-find's arrays
        PhaseClock clk{6};
        double ms[4] = {};      // init + hook, flatten, sizes + summary, copies
        bool valid = false;     // label / size / summary describe the roadmap as it stands: kept until it changes
        DevBuf<uint32_t> parent, label, count, size;
        DevBuf<unsigned long long> summary;
    } cc;
    struct {   // oxhip_prm_prune: its masks and scans (it labels into cc's arrays and compacts into `spare`)
        PhaseClock clk{10};
        double ms[5] = {};   // masks, components, scans, move entries, move states
        DevBuf<uint8_t> keep, mask, ekeep;
        DevBuf<uint32_t> pos, epos, kept;
        DevBuf<int32_t> index;
    } prune;
    struct {   // oxhip_prm_batch_simplify_paths: the last batch's answered paths, subdivided and shortcut
        PhaseClock clk{8};
        double ms[4] = {};   // upload + subdivide, pair matrix, DP, copies
        bool valid = false;  // the results below belong to the current batch: dropped with it (drop_derived, stage_batch)
        uint32_t rounds = 0;
        std::vector<uint64_t> soff, checks;          // [Q + 1] row offsets of the simplified paths, [Q]
        std::vector<uint32_t> idx;                   // dense indices of their rows
        std::vector<double> rows, raw_cost, simp_cost;
        // d_: the raw paths of the batch, then the per-round workspace
        DevBuf<uint64_t> d_off, d_doff, d_woff, d_bits, d_checks, d_soff;
        DevBuf<uint32_t> d_len, d_par, d_idx, d_simp_len, d_out_idx;
        DevBuf<double> d_rows, d_dense, d_cost, d_raw, d_simp, d_out_rows;
    } simplify;
};

namespace {

int32_t read_state(oxhip_prm* h, PrmState& st) {
    HIP_TRY(hipMemcpyAsync(&st, h->work.state.p, sizeof(PrmState), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return OXHIP_OK;
}

int32_t write_state(oxhip_prm* h, const PrmState& st) {
    HIP_TRY(hipMemcpyAsync(h->work.state.p, &st, sizeof(PrmState), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return OXHIP_OK;
}

// ---- the one place that names the space: which launcher, and whether a radius travels as given or as its squared threshold
void launch_pairs(oxhip_prm* h, uint32_t j0, uint32_t j1) {   // the k-nearest variant searches its per-row radii (knn_row_radii)
    if (h->so3) launch_prm_so3_pairs(h->args, j0, j1, h->so3_lo, h->so3_hi, h->cfg.connection_radius, h->stream);
    else if (h->cfg.knn_k) launch_prm_pairs(h->dp, h->args, j0, j1, std::numeric_limits<double>::infinity(), h->stream, h->knn.thr.p, h->knn.thr32.p);
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
    for (uint32_t k = 0; k < h->cfg.dim; ++k) qdp.filt_abs = std::fmax(qdp.filt_abs, 1e-9 * std::fabs(h->single.query.start[k]));
    launch_prm_query(h->so3, qdp, h->args, h->rm.n, h->single.query, near_threshold(h), h->single.flags.p, h->single.start_valid.p, h->stream);
}
void launch_batch_flags(oxhip_prm* h, const PrmBatchArgs& b) { launch_prm_batch_flags(h->so3, h->dp, b, near_threshold(h), h->stream); }
// a planted roadmap's fl32 shadow, which the R^n pair search screens with (the SO(3) pair search screens nothing)
void launch_planted_shadow(oxhip_prm* h, uint32_t n) {
    if (!h->so3) launch_prm_shadow(h->rm.ms.p, h->rm.ms32.p, (uint64_t)n * h->cfg.dim, h->stream);
}
// the re-check's pair list: R^n (entry, u, v) for its own check kernel; SO(3) construction's candidate layout, with a key array
// and a counter of the re-check's own, for construction's edge kernel
int32_t reserve_reval_pairs(oxhip_prm* h, uint32_t pair_cap) {
    if (!h->so3) { HIP_TRY(h->reval.pairs.reserve(pair_cap)); return OXHIP_OK; }
    HIP_TRY(h->reval.cand.reserve(pair_cap)); HIP_TRY(h->reval.keys.reserve(2 * (size_t)pair_cap)); HIP_TRY(h->reval.state.reserve(1));
    HIP_TRY(hipMemsetAsync(h->reval.state.p, 0, sizeof(PrmState), h->stream));
    return OXHIP_OK;
}
uint2* reval_cand(oxhip_prm* h) { return h->so3 ? h->reval.cand.p : nullptr; }   // (the emit launcher fills reval.pairs when this is null)
// check_motion(from = u, to = v) per pair of the list; a valid one keeps its two entries
int32_t launch_reval_edges(oxhip_prm* h, uint32_t n_pairs, uint32_t n, uint32_t n_old) {
    if (!h->so3) {
        launch_prm_reval_check(h->dp, h->rm.ms.p, h->rm.offsets.p, h->rm.nbrs.p, n, n_old, h->reval.pairs.p, n_pairs, h->reval.keep.p, h->stream);
    } else if (n_pairs) {
        PrmArgs a = h->args;   // construction's kernel, the re-check's buffers: nothing of construction's workspace is touched
        a.cand = h->reval.cand.p; a.keys = h->reval.keys.p; a.state = h->reval.state.p;
        launch_edges(h, a, n_pairs);   // both directed keys of every valid pair
        HIP_TRY(hipGetLastError());
        launch_prm_reval_keys(h->reval.keys.p, h->reval.state.p, 2 * n_pairs, prm_key_shift(h->args.cap), h->rm.offsets.p, h->rm.nbrs.p, n, h->reval.keep.p,
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
    h->single.query = PrmQuery{};
    std::memcpy(h->single.query.start, start, dim * sizeof(double));
    std::memcpy(h->single.query.goal_c, goal_centre, dim * sizeof(double));
    h->single.query.goal_thr = goal_threshold(h, goal_radius);
    return OXHIP_OK;
}

// the kernels' view of the milestones, re-derived from the roadmap: whatever replaces one of its buffers ends here
void bind_roadmap(oxhip_prm* h) { h->args.ms = h->rm.ms.p; h->args.ms32 = h->rm.ms32.p; }

// What is derived from the roadmap as it was -- the host copy, the single query's sets, the last batch's results (batch.valid) and their shortcut (simplify.valid), the
// edge weights (shortest.w_valid), the component labels (cc.valid) -- and so is gone when it changes: every function that changes `rm` ends here.
void drop_derived(oxhip_prm* h) {
    h->single.host_copy = false;
    h->single.h_offsets.clear(); h->single.h_nbrs.clear(); h->single.h_states.clear();
    h->single.start_conn.clear(); h->single.goal_idx.clear();
    h->batch.valid = h->simplify.valid = h->shortest.w_valid = h->cc.valid = false;
}

// setup: no roadmap; set_roadmap: one of n milestones that this handle did not sample.  The samples and the stream position
// belonged to the roadmap that went.
void clear_roadmap(oxhip_prm* h, uint32_t n = 0, uint32_t n_keys = 0) {
    h->rm.n = n; h->rm.n_keys = n_keys;
    h->sampler.n_samples = 0; h->sampler.redraw_batches = 0; h->sampler.pos_valid = false;
    drop_derived(h);
}

// One round of the space's parallel sampler from stream word st.draws on.  R^n: m samples.  SO(3) (prm_so3.hip): m rejection
// attempts, attempt a at stream word pos0 + 4 a.
int32_t sample_round(oxhip_prm* h, const PrmState& st, uint32_t m) {
    if (h->so3) {
        HIP_TRY(h->sampler.abits.reserve((m + 63) / 64)); HIP_TRY(h->sampler.acnt.reserve((m + 63) / 64));
        PrmSo3Spec sp{};
        sp.pos0 = st.draws; sp.m = m;
        sp.tmp = h->sampler.tmp.p; sp.vbits = h->sampler.vbits.p; sp.abits = h->sampler.abits.p; sp.voff = h->sampler.off.p; sp.acnt = h->sampler.acnt.p;
        sp.redraw_flag = h->sampler.flag.p; sp.result = h->work.state.p;
        launch_prm_so3_sample(h->dp, h->args, sp, st.n_milestones, h->stream);
    } else {
        PrmSpec sp{};
        sp.pos0 = st.draws; sp.m = m;
        sp.tmp = h->sampler.tmp.p; sp.vbits = h->sampler.vbits.p; sp.wave_off = h->sampler.off.p;
        sp.redraw_flag = h->sampler.flag.p; sp.result = h->work.state.p;   // the scan kernel advances the device state
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

// Draw samples until `target` milestones exist or `max_samples` were drawn, timed into t's sample phase: rounds of the parallel sampler, sized
// by the observed rate of milestones per sample (SO(3): per attempt; its kernel stops at args.max_samples itself, so its rounds are not clamped).
int32_t sample_until(oxhip_prm* h, PrmBuildTally& t, PrmState& st, uint32_t target, uint64_t max_samples) {
    constexpr uint64_t kRoundMax = 1ull << 22;
    const bool so3 = h->so3;
    HIP_TRY(t.clk.mark(kBegin, h->stream));
    h->args.n_target = target;
    if (so3) h->args.max_samples = max_samples;
    while (st.n_milestones < target && st.n_samples < max_samples) {
        const uint32_t need = target - st.n_milestones;
        uint64_t want = std::min((uint64_t)((double)need / h->sampler.valid_rate * 1.02) + 256, kRoundMax);
        if (!so3) want = std::min(want, max_samples - st.n_samples);
        const uint32_t m = (uint32_t)want, nw = (m + 63) / 64;
        HIP_TRY(h->sampler.tmp.reserve((size_t)m * h->cfg.dim)); HIP_TRY(h->sampler.flag.reserve(1));   // (SO(3): dim is 4)
        HIP_TRY(h->sampler.vbits.reserve(nw)); HIP_TRY(h->sampler.off.reserve(nw));
        HIP_TRY(hipMemsetAsync(h->sampler.flag.p, 0, sizeof(uint32_t), h->stream));
        OX_TRY(sample_round(h, st, m));
        PrmState after{};
        uint32_t flag = 0;
        HIP_TRY(hipMemcpyAsync(&after, h->work.state.p, sizeof(PrmState), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(&flag, h->sampler.flag.p, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        if (flag != 0) { OX_TRY(flagged_round(h, st, m)); continue; }
        const double got = (double)(after.n_milestones - st.n_milestones), drawn = so3 ? (double)m : (double)(after.n_samples - st.n_samples);
        h->sampler.valid_rate = std::max(so3 ? 1e-6 : 1.0 / 64.0, std::min(1.0, (got + 1.0) / (drawn + 1.0)));
        st = after;
    }
    HIP_TRY(t.clk.mark(kEnd, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    t.ms[0] += t.clk.ms(kBegin, kEnd);
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
    if (h->single.host_copy) return OXHIP_OK;
    const uint32_t n = h->rm.n, n_keys = h->rm.n_keys;
    h->single.h_offsets.assign((size_t)n + 1, 0);
    h->single.h_nbrs.assign(n_keys, 0);
    h->single.h_states.assign((size_t)n * h->cfg.dim, 0.0);
    if (n) {
        HIP_TRY(hipMemcpyAsync(h->single.h_offsets.data(), h->rm.offsets.p, ((size_t)n + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        if (n_keys) HIP_TRY(hipMemcpyAsync(h->single.h_nbrs.data(), h->rm.nbrs.p, (size_t)n_keys * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(h->single.h_states.data(), h->rm.ms.p, (size_t)n * h->cfg.dim * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    h->single.host_copy = true;
    return OXHIP_OK;
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

// the stream and the buffers that live as long as the handle (its clocks were made with it); the first error wins
int32_t alloc_prm(oxhip_prm* h) {
    const uint32_t dim = h->cfg.dim, cap = ((h->cfg.max_milestones + 1023u) / 1024u) * 1024u;
    hipError_t e = hipSuccess;
    auto chk = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    chk(oxhip_stream_acquire(h->cfg.device, &h->stream));
    for (const PhaseClock* c : {&h->built.clk, &h->single.clk, &h->batch.clk, &h->shortest.clk, &h->reval.clk, &h->grow.tally.clk, &h->cc.clk, &h->prune.clk, &h->simplify.clk})
        chk(c->made);   // an event that could not be made refuses the create, as a buffer does
    chk(h->rm.ms.alloc((size_t)dim * cap));
    if (!h->so3) chk(h->rm.ms32.alloc((size_t)dim * cap));   // (the SO(3) pair search screens nothing)
    chk(h->work.state.alloc(1));
    chk(h->single.flags.alloc(cap));
    chk(h->single.start_valid.alloc(1));
    chk(h->rm.offsets.alloc((size_t)cap + 1));
    if (e != hipSuccess) return alloc_failed(e);
    bind_roadmap(h);
    h->args.state = h->work.state.p; h->args.cap = cap; h->args.stream = h->cfg.stream;
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
    HIP_TRY(h->knn.thr.reserve(h->args.cap)); HIP_TRY(h->knn.thr32.reserve(h->args.cap));
    HIP_TRY(hipMemcpyAsync(h->knn.thr.p, thr.data(), thr.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->knn.thr32.p, thr32.data(), thr32.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return OXHIP_OK;
}

// pairs (j in [n_done, n_now), i < j) within the connection radius, into h->work.cand; st.n_cand counts them
int32_t find_pairs(oxhip_prm* h, PrmBuildTally& t, PrmState& st, uint32_t n_done, uint32_t n_now) {
    if (h->work.cand.n == 0) HIP_TRY(h->work.cand.alloc(std::min<size_t>(std::max<size_t>(1u << 20, (size_t)64 * h->cfg.max_milestones), (size_t)1 << 28)));
    for (;;) {
        h->args.cand = h->work.cand.p;
        h->args.cand_cap = (uint32_t)h->work.cand.n;
        st.n_cand = 0;
        OX_TRY(write_state(h, st));
        HIP_TRY(t.clk.mark(kBegin, h->stream));
        launch_pairs(h, n_done, n_now);
        HIP_TRY(hipGetLastError());
        HIP_TRY(t.clk.mark(kEnd, h->stream));
        PrmState s2{};
        OX_TRY(read_state(h, s2));
        t.ms[1] += t.clk.ms(kBegin, kEnd);
        st.n_cand = s2.n_cand;
        if (st.n_cand <= h->args.cand_cap) break;
        // candidate buffer too small: the kernel kept counting, so the exact need is known; run again
        if (st.n_cand > 0x7FFFFFFFull) return fail(OXHIP_ERR_CAPACITY, "more than 2^31 in-radius pairs in one round");
        HIP_TRY(h->work.cand.alloc((size_t)st.n_cand));
    }
    t.candidates += st.n_cand;
    return OXHIP_OK;
}

// k-nearest variant: each row's k nearest among its candidates (sorted by (j, i)), the exact search for rows that fell short.
// The selected pairs replace the candidates as what the edge step reads: `pairs` and st.n_cand.
int32_t knn_select(oxhip_prm* h, PrmBuildTally& t, PrmState& st, uint32_t n_done, uint32_t n_now, uint2*& pairs) {
    const uint32_t nc = (uint32_t)st.n_cand, rows = n_now - n_done, knn_k = h->cfg.knn_k;
    HIP_TRY(h->knn.keys.reserve(nc + 1)); HIP_TRY(h->knn.sorted.reserve(nc + 1)); HIP_TRY(h->knn.dist.reserve(nc + 1));
    HIP_TRY(h->knn.sel.reserve((size_t)rows * knn_k)); HIP_TRY(h->knn.failed.reserve(rows)); HIP_TRY(h->knn.counters.reserve(2));
    size_t tb = 0;
    if (nc) {
        HIP_TRY(prm_sort_keys(nullptr, tb, h->knn.keys.p, h->knn.sorted.p, nc, h->args.cap, h->stream));
        HIP_TRY(h->work.sort_tmp.reserve(tb));
    }
    HIP_TRY(t.clk.mark(kBegin, h->stream));
    HIP_TRY(hipMemsetAsync(h->knn.counters.p, 0, 2 * sizeof(uint32_t), h->stream));
    launch_prm_knn_keys(h->args, nc, h->knn.keys.p, h->stream);
    if (nc) HIP_TRY(prm_sort_keys(h->work.sort_tmp.p, tb, h->knn.keys.p, h->knn.sorted.p, nc, h->args.cap, h->stream));
    launch_prm_knn_select(h->dp, h->args, h->knn.sorted.p, h->knn.dist.p, nc, n_done, n_now, knn_k, h->knn.sel.p, h->knn.counters.p,
                          h->knn.failed.p, h->stream);
    HIP_TRY(hipGetLastError());
    uint32_t cnt[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(cnt, h->knn.counters.p, sizeof cnt, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (cnt[1]) {
        launch_prm_knn_brute(h->dp, h->args, h->knn.failed.p, cnt[1], knn_k, h->knn.sel.p, h->knn.counters.p, h->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(cnt, h->knn.counters.p, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        t.exact_rows += cnt[1];
    }
    HIP_TRY(t.clk.mark(kEnd, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    t.ms[1] += t.clk.ms(kBegin, kEnd);
    st.n_cand = cnt[0];
    pairs = h->knn.sel.p;
    return OXHIP_OK;
}

// room for the keys this round can add, at most 2 per pair: growth keeps the keys of the rounds before
int32_t reserve_keys(oxhip_prm* h, const PrmState& st) {
    const uint64_t need = (uint64_t)st.n_keys + 2ull * st.n_cand;
    if (need > 0xFFFFFFFFull) return fail(OXHIP_ERR_CAPACITY, "more than 2^32 directed edges");
    if (need <= h->work.keys.n) return OXHIP_OK;
    DevBuf<uint64_t> bigger;
    HIP_TRY(bigger.alloc(std::max<size_t>((size_t)need, h->work.keys.n * 2)));
    if (st.n_keys) HIP_TRY(hipMemcpyAsync(bigger.p, h->work.keys.p, (size_t)st.n_keys * sizeof(uint64_t), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->work.keys.swap(bigger);
    h->args.keys = h->work.keys.p;
    return OXHIP_OK;
}

// check_motion per pair of `pairs`; the kernel appends the keys of the edges and st comes back with their count
int32_t check_edges(oxhip_prm* h, PrmBuildTally& t, PrmState& st, uint2* pairs) {
    PrmArgs a = h->args;
    a.cand = pairs;
    HIP_TRY(t.clk.mark(kBegin, h->stream));
    launch_edges(h, a, (uint32_t)st.n_cand);
    HIP_TRY(hipGetLastError());
    HIP_TRY(t.clk.mark(kEnd, h->stream));
    OX_TRY(read_state(h, st));
    t.ms[2] += t.clk.ms(kBegin, kEnd);
    return OXHIP_OK;
}

// sort the directed keys -> every node's neighbours in ascending order (the reference's `edges`), as CSR
int32_t build_csr(oxhip_prm* h, PrmBuildTally& t, uint32_t n, uint32_t n_keys) {
    size_t tmp_bytes = 0;
    if (n_keys) {
        // (re)size the sort's buffers before the timed region: hipMalloc is a blocking call
        HIP_TRY(h->work.keys_sorted.reserve(n_keys)); HIP_TRY(h->rm.nbrs.reserve(n_keys));
        HIP_TRY(prm_sort_keys(nullptr, tmp_bytes, h->work.keys.p, h->work.keys_sorted.p, n_keys, h->args.cap, h->stream));
        HIP_TRY(h->work.sort_tmp.reserve(tmp_bytes));
    }
    HIP_TRY(t.clk.mark(kBegin, h->stream));
    if (n_keys) {
        HIP_TRY(prm_sort_keys(h->work.sort_tmp.p, tmp_bytes, h->work.keys.p, h->work.keys_sorted.p, n_keys, h->args.cap, h->stream));
        launch_prm_csr(h->work.keys_sorted.p, n_keys, n, h->args.cap, h->rm.offsets.p, h->rm.nbrs.p, h->stream);
        HIP_TRY(hipGetLastError());
    } else {
        HIP_TRY(hipMemsetAsync(h->rm.offsets.p, 0, ((size_t)n + 1) * sizeof(uint32_t), h->stream));
    }
    HIP_TRY(t.clk.mark(kEnd, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    t.ms[3] = t.clk.ms(kBegin, kEnd);
    return OXHIP_OK;
}

// start validity, start connections and goal milestones of h->single.query (prm.rs:243-264), on the device
int32_t query_sets(oxhip_prm* h, std::vector<uint8_t>& flags) {
    const uint32_t n = h->rm.n;
    uint32_t start_valid = 0;
    HIP_TRY(h->single.clk.mark(kBegin, h->stream));
    launch_query(h);
    HIP_TRY(hipGetLastError());
    HIP_TRY(h->single.clk.mark(kEnd, h->stream));
    flags.assign(n, 0);
    HIP_TRY(hipMemcpyAsync(flags.data(), h->single.flags.p, n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(&start_valid, h->single.start_valid.p, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->single.ms[0] = h->single.clk.ms(kBegin, kEnd);
    if (!start_valid) return fail(OXHIP_ERR_INVALID_START_STATE, "start state is in collision");  // prm.rs:243-246
    for (uint32_t i = 0; i < n; ++i) {
        if (flags[i] & 1) h->single.start_conn.push_back(i);   // prm.rs:249-256
        if (flags[i] & 2) h->single.goal_idx.push_back(i);     // prm.rs:259-264
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
    OX_TRY(upload(h->obs.sph_c, c, h->stream));
    OX_TRY(upload(h->obs.sph_thr, thr, h->stream));
    OX_TRY(upload(h->obs.sph_r, std::vector<double>(radii, radii + n), h->stream));
    h->dp.n_spheres = n; h->dp.sph_c = h->obs.sph_c.p; h->dp.sph_thr = h->obs.sph_thr.p; h->dp.sph_r = h->obs.sph_r.p;
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
    OX_TRY(upload(h->obs.box_lo, l, h->stream));
    OX_TRY(upload(h->obs.box_hi, u, h->stream));
    h->dp.n_boxes = n; h->dp.box_lo = h->obs.box_lo.p; h->dp.box_hi = h->obs.box_hi.p;
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
    if (h->rm.n != 0) return OXHIP_OK;  // prm.rs:106-113: "Roadmap already constructed"
    OX_TRY(select_device(h->cfg.device));
    const auto t0 = std::chrono::steady_clock::now();
    const bool has_timeout = h->cfg.timeout > 0.0 && std::isfinite(h->cfg.timeout);
    const uint32_t n_max = h->cfg.max_milestones, knn_k = h->cfg.knn_k;
    // 0 = "unlimited", which still has to end when (almost) no sample is valid: 4096 draws per requested milestone
    const uint64_t max_samples = h->cfg.max_samples ? h->cfg.max_samples : 4096ull * n_max + (1ull << 22);
    PrmBuildTally& t = h->built;
    t.reset();
    for (double& q : h->single.ms) q = 0.0;   // oxhip_prm_last_timing's six entries start over together
    PrmState st{};
    OX_TRY(write_state(h, st));
    h->sampler.valid_rate = 1.0;
    // without a wall clock the roadmap is built in one round; with one, in doubling rounds with the
    // clock read in between (the reference reads it before every sample, prm.rs:118)
    uint32_t target = has_timeout ? std::min<uint32_t>(n_max, 4096u) : n_max;
    uint32_t n_done = 0;  // milestones whose pairs are already connected
    for (;;) {
        OX_TRY(sample_until(h, t, st, target, max_samples));
        const uint32_t n_now = st.n_milestones;
        // thr_conn >= 0 <=> connection_radius > 0 (sqrt_lt_threshold; NaN was refused), in either space: a radius <= 0 takes no pair
        if (n_now > n_done && n_now >= 2 && (h->thr_conn >= 0.0 || knn_k)) {
            if (knn_k) OX_TRY(knn_row_radii(h, st, n_done, n_now));
            OX_TRY(find_pairs(h, t, st, n_done, n_now));
            uint2* pairs = h->work.cand.p;
            if (knn_k) OX_TRY(knn_select(h, t, st, n_done, n_now, pairs));
            OX_TRY(reserve_keys(h, st));
            OX_TRY(check_edges(h, t, st, pairs));
        }
        n_done = n_now;
        if (n_now < target) break;                       // max_samples exhausted
        if (n_now >= n_max) break;
        if (has_timeout && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > h->cfg.timeout)
            break;                                       // prm.rs:118-120
        target = target > n_max / 2 ? n_max : target * 2;
    }
    OX_TRY(build_csr(h, t, st.n_milestones, st.n_keys));
    h->rm.n = st.n_milestones;
    h->rm.n_keys = st.n_keys;
    h->sampler.n_samples = st.n_samples;
    h->sampler.redraw_batches = st.redraw_batches;
    h->sampler.pos_valid = true; h->sampler.pos_stream = h->cfg.stream; h->sampler.pos_draws = st.draws;   // where oxhip_prm_grow_roadmap continues
    drop_derived(h);   // (the host copy is fetched by the first get_roadmap / solve)
    return OXHIP_OK;
}

int32_t oxhip_prm_knn_exact_rows(oxhip_prm* h, uint32_t* rows) {
    if (!h || !rows) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    *rows = h->built.exact_rows;
    return OXHIP_OK;
}

int32_t oxhip_prm_get_sizes(oxhip_prm* h, uint32_t* n_milestones, uint64_t* n_edge_entries, uint64_t* n_samples) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (n_milestones) *n_milestones = h->rm.n;
    if (n_edge_entries) *n_edge_entries = h->rm.n_keys;
    if (n_samples) *n_samples = h->sampler.n_samples;
    return OXHIP_OK;
}

// get_roadmap (prm.rs:82-84)
int32_t oxhip_prm_get_roadmap(oxhip_prm* h, double* states, uint32_t cap_nodes, uint64_t* offsets, uint32_t* neighbours,
                              uint64_t cap_entries) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (h->rm.n) {
        OX_TRY(select_device(h->cfg.device));
        OX_TRY(fetch_roadmap(h));
    }
    if ((states || offsets) && cap_nodes < h->rm.n) return fail(OXHIP_ERR_CAPACITY, "roadmap buffers too small");
    if (neighbours && cap_entries < h->single.h_nbrs.size()) return fail(OXHIP_ERR_CAPACITY, "neighbour buffer too small");
    if (states && h->rm.n) std::memcpy(states, h->single.h_states.data(), h->single.h_states.size() * sizeof(double));
    if (offsets) {
        for (uint32_t i = 0; i <= h->rm.n; ++i) offsets[i] = h->single.h_offsets.empty() ? 0 : h->single.h_offsets[i];
    }
    if (neighbours && !h->single.h_nbrs.empty()) std::memcpy(neighbours, h->single.h_nbrs.data(), h->single.h_nbrs.size() * sizeof(uint32_t));
    return OXHIP_OK;
}

// Planner::solve (prm.rs:227-307)
int32_t oxhip_prm_solve(oxhip_prm* h, double timeout_s, double* path, uint32_t cap_states, uint32_t* len) {
    if (!h || !len) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    *len = 0;
    h->single.start_conn.clear();
    h->single.goal_idx.clear();
    if (!h->is_setup) return fail(OXHIP_ERR_PLANNER_UNINITIALISED, "setup() was not called");      // prm.rs:229-236
    if (h->rm.n == 0) return fail(OXHIP_ERR_UNSAMPLED_STATE_SPACE, "construct_roadmap() left no milestones");  // prm.rs:239-241
    OX_TRY(select_device(h->cfg.device));
    OX_TRY(fetch_roadmap(h));
    std::vector<uint8_t> flags;
    OX_TRY(query_sets(h, flags));
    const auto t0 = std::chrono::steady_clock::now();
    const bool has_timeout = timeout_s > 0.0 && std::isfinite(timeout_s);
    std::vector<uint32_t> chain;   // goal milestone ... root connection
    const PrmBfs found = prm_bfs_path(h->single.h_offsets, h->single.h_nbrs, flags, h->single.start_conn, has_timeout ? timeout_s : std::numeric_limits<double>::infinity(), chain);
    if (found == PrmBfs::empty_set) return fail(OXHIP_ERR_NO_SOLUTION_FOUND, "start or goal does not connect to the roadmap");  // prm.rs:266-268
    h->single.ms[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (found == PrmBfs::timed_out) return fail(OXHIP_ERR_TIMEOUT, "graph search timed out");  // prm.rs:285-287
    if (found == PrmBfs::unreachable) return fail(OXHIP_ERR_NO_SOLUTION_FOUND, "goal is not reachable on the roadmap");  // prm.rs:304
    // [start] ++ (root connection ... goal milestone)
    const uint32_t dim = h->cfg.dim;
    *len = (uint32_t)chain.size() + 1;
    if (!path) return OXHIP_OK;
    if (*len > cap_states) return fail(OXHIP_ERR_CAPACITY, "path buffer too small");
    std::memcpy(path, h->single.query.start, dim * sizeof(double));
    for (size_t j = 0; j < chain.size(); ++j)
        std::memcpy(path + (j + 1) * dim, h->single.h_states.data() + (size_t)chain[chain.size() - 1 - j] * dim, dim * sizeof(double));
    return OXHIP_OK;
}

int32_t oxhip_prm_get_query_sets(oxhip_prm* h, uint32_t* start_connections, uint32_t cap_start, uint32_t* n_start,
                                 uint32_t* goal_indices, uint32_t cap_goal, uint32_t* n_goal) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (n_start) *n_start = (uint32_t)h->single.start_conn.size();
    if (n_goal) *n_goal = (uint32_t)h->single.goal_idx.size();
    if (start_connections) {
        if (cap_start < h->single.start_conn.size()) return fail(OXHIP_ERR_CAPACITY, "start_connections buffer too small");
        if (!h->single.start_conn.empty()) std::memcpy(start_connections, h->single.start_conn.data(), h->single.start_conn.size() * sizeof(uint32_t));
    }
    if (goal_indices) {
        if (cap_goal < h->single.goal_idx.size()) return fail(OXHIP_ERR_CAPACITY, "goal_indices buffer too small");
        if (!h->single.goal_idx.empty()) std::memcpy(goal_indices, h->single.goal_idx.data(), h->single.goal_idx.size() * sizeof(uint32_t));
    }
    return OXHIP_OK;
}

int32_t oxhip_prm_last_timing(oxhip_prm* h, double* phase_ms, uint64_t* n_candidates, uint32_t* redraw_batches) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (phase_ms) for (int i = 0; i < 6; ++i) phase_ms[i] = i < 4 ? h->built.ms[i] : h->single.ms[i - 4];
    if (n_candidates) *n_candidates = h->built.candidates;
    if (redraw_batches) *redraw_batches = h->sampler.redraw_batches;
    return OXHIP_OK;
}

}  // extern "C"

// ---- a batch of queries on the roadmap as it stands: prm.rs:243-307 per query, all of it on the device

namespace {

// the arguments of one round of the last batch: queries [q0, q0 + n_chunk) in the workspace rows [0, n_chunk)
PrmBatchArgs batch_args(oxhip_prm* h, uint32_t q0, uint32_t n_chunk, uint32_t res_cap) {
    PrmBatchArgs b{};
    b.ms = h->rm.ms.p; b.offsets = h->rm.offsets.p; b.nbrs = h->rm.nbrs.p;
    b.starts = h->batch.d_starts.p; b.goals = h->batch.d_goals.p; b.goal_thr = h->batch.d_thr.p; b.filt = h->batch.d_filt.p;
    b.flags = h->batch.d_flags.p; b.start_valid = h->batch.d_start_valid.p; b.parent = h->batch.d_parent.p; b.queue = h->batch.d_queue.p;
    b.status = (int32_t*)h->batch.d_res.p; b.path_len = h->batch.d_res.p + res_cap; b.goal_node = (int32_t*)(h->batch.d_res.p + 2 * (size_t)res_cap);
    b.n_start = h->batch.d_res.p + 3 * (size_t)res_cap; b.n_goal = h->batch.d_res.p + 4 * (size_t)res_cap;
    b.n = h->rm.n; b.stride = (h->rm.n + 63u) & ~63u; b.dim = h->cfg.dim; b.q0 = q0; b.n_chunk = n_chunk;
    return b;
}

PrmShortestArgs shortest_args(oxhip_prm* h, int32_t mode) {
    PrmShortestArgs a{};
    a.w = h->shortest.w_edges.p; a.label = h->shortest.d_label.p; a.stamp = h->shortest.d_stamp.p; a.cost = h->shortest.d_cost.p; a.rounds = h->shortest.d_rounds.p;
    a.relaxed = h->shortest.d_relaxed.p; a.mode = (uint32_t)mode;
    return a;
}

// the distances of the roadmap's CSR entries, once per roadmap (distance weights only)
int32_t ensure_edge_weights(oxhip_prm* h) {
    if (h->shortest.w_valid) return OXHIP_OK;
    HIP_TRY(h->shortest.w_edges.reserve(h->rm.n_keys));
    HIP_TRY(h->shortest.clk.mark(kBegin, h->stream));
    launch_prm_shortest_weights(h->so3, h->cfg.dim, h->rm.ms.p, h->rm.offsets.p, h->rm.nbrs.p, h->rm.n, h->rm.n_keys, h->shortest.w_edges.p, h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(h->shortest.clk.mark(kEnd, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->shortest.ms[0] = h->shortest.clk.ms(kBegin, kEnd);
    h->shortest.w_valid = true;
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
    if (h->rm.n == 0) return fail(OXHIP_ERR_UNSAMPLED_STATE_SPACE, "construct_roadmap() left no milestones");  // prm.rs:239-241
    const uint32_t dim = h->cfg.dim;
    OX_TRY(check_query_points(starts, goal_centres, (size_t)Q * dim));
    OX_TRY(select_device(h->cfg.device));
    h->batch.valid = h->simplify.valid = false;
    h->batch.rounds = 0;
    h->batch.mode = mode;
    for (double& t : h->batch.ms) t = 0.0;
    for (double& t : h->shortest.ms) t = 0.0;
    h->shortest.cost.assign(mode < 0 ? 0 : Q, std::numeric_limits<double>::infinity());
    h->shortest.rounds.assign(mode < 0 ? 0 : Q, 0u);
    h->shortest.relaxed.assign(mode < 0 ? 0 : Q, 0ull);
    h->batch.starts.assign(starts, starts + (size_t)Q * dim);
    h->batch.goals.assign(goal_centres, goal_centres + (size_t)Q * dim);
    h->batch.thr.resize(Q); h->batch.filt.resize(Q);
    for (uint32_t q = 0; q < Q; ++q) {
        h->batch.thr[q] = goal_threshold(h, goal_radii[q]);
        double f = h->dp.filt_abs;   // the start may lie anywhere: the filter's absolute margin with this start in play
        for (uint32_t k = 0; k < dim; ++k) f = std::fmax(f, 1e-9 * std::fabs(starts[(size_t)q * dim + k]));
        h->batch.filt[q] = f;
    }
    h->batch.status.assign(Q, OXHIP_ERR_TIMEOUT);
    h->batch.goal_node.assign(Q, -1);
    h->batch.len.assign(Q, 0); h->batch.nstart.assign(Q, 0); h->batch.ngoal.assign(Q, 0);
    h->batch.off.assign((size_t)Q + 1, 0);
    h->batch.nodes.clear(); h->batch.rows.clear();
    if (!Q) return OXHIP_OK;
    HIP_TRY(h->batch.d_starts.reserve((size_t)Q * dim)); HIP_TRY(h->batch.d_goals.reserve((size_t)Q * dim));
    HIP_TRY(h->batch.d_thr.reserve(Q)); HIP_TRY(h->batch.d_filt.reserve(Q));
    HIP_TRY(hipMemcpyAsync(h->batch.d_starts.p, h->batch.starts.data(), (size_t)Q * dim * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->batch.d_goals.p, h->batch.goals.data(), (size_t)Q * dim * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->batch.d_thr.p, h->batch.thr.data(), (size_t)Q * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->batch.d_filt.p, h->batch.filt.data(), (size_t)Q * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return OXHIP_OK;
}

// The size of a round -- 9 bytes per query and milestone (21 for shortest paths), sized to keep the workspace within 1 GiB -- and
// every buffer a round of that size needs; distance weights: the roadmap's edge weights, once per roadmap
int32_t reserve_batch_workspace(oxhip_prm* h, BatchRun& br, uint32_t chunk_queries) {
    br.stride = (h->rm.n + 63u) & ~63u;
    uint32_t chunk = chunk_queries ? chunk_queries : (uint32_t)std::max<uint64_t>(1, (1ull << 30) / (batch_bytes_per_node(br.mode) * br.stride));
    br.chunk = chunk = std::min(std::min(chunk, br.Q), 65535u);
    const size_t cells = (size_t)chunk * br.stride;
    if (br.mode >= 0) {
        HIP_TRY(h->shortest.d_label.reserve(cells)); HIP_TRY(h->shortest.d_stamp.reserve(cells));
        HIP_TRY(h->shortest.d_cost.reserve(chunk)); HIP_TRY(h->shortest.d_rounds.reserve(chunk)); HIP_TRY(h->shortest.d_relaxed.reserve(chunk));
    }
    if (br.mode == 0) OX_TRY(ensure_edge_weights(h));
    br.sa = shortest_args(h, br.mode);
    HIP_TRY(h->batch.d_flags.reserve(cells)); HIP_TRY(h->batch.d_parent.reserve(cells)); HIP_TRY(h->batch.d_queue.reserve(cells));
    HIP_TRY(h->batch.d_start_valid.reserve(chunk)); HIP_TRY(h->batch.d_off.reserve(chunk));
    HIP_TRY(h->batch.d_res.reserve(5 * (size_t)chunk));   // (the getters take d_res.n / 5 as a round's row count: never below this one)
    br.group = prm_batch_group(h->rm.n, h->rm.n_keys);
    br.res.resize(5 * (size_t)chunk); br.off.resize(chunk);
    return OXHIP_OK;
}

// flags, initial labels, label rounds and tight levels of the queries of `b`; `timed`: a batch's round, which marks its clock between
int32_t launch_shortest(oxhip_prm* h, const PrmBatchArgs& b, const PrmShortestArgs& sa, uint32_t group, bool timed) {
    launch_batch_flags(h, b);
    launch_prm_shortest_init(h->so3, b, sa, h->stream);
    if (timed) HIP_TRY(h->batch.clk.mark(kFlagsEnd, h->stream));
    launch_prm_shortest_labels(b, sa, group, h->stream);
    HIP_TRY(hipGetLastError());
    if (timed) HIP_TRY(h->batch.clk.mark(kLabelsEnd, h->stream));
    launch_prm_shortest_levels(b, sa, group, h->stream);
    HIP_TRY(hipGetLastError());
    return OXHIP_OK;
}

// one round on the device: the query sets, the search, and its results copied into `br` (the search's own figures: to their queries)
int32_t run_round(oxhip_prm* h, BatchRun& br, const PrmBatchArgs& b) {
    const uint32_t c = b.n_chunk, q0 = b.q0;
    HIP_TRY(hipMemsetAsync(h->batch.d_parent.p, 0xFF, (size_t)c * br.stride * sizeof(uint32_t), h->stream));
    PhaseClock& clk = h->batch.clk;
    HIP_TRY(clk.mark(kRoundBegin, h->stream));
    if (br.mode < 0) {
        launch_batch_flags(h, b);
        HIP_TRY(clk.mark(kFlagsEnd, h->stream));
        launch_prm_batch_search(b, br.group, h->stream);
        HIP_TRY(hipGetLastError());
    } else {
        OX_TRY(launch_shortest(h, b, br.sa, br.group, true));
    }
    HIP_TRY(clk.mark(kSearchEnd, h->stream));
    HIP_TRY(hipMemcpyAsync(br.res.data(), h->batch.d_res.p, 5 * (size_t)br.chunk * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    if (br.mode >= 0) {
        HIP_TRY(hipMemcpyAsync(h->shortest.cost.data() + q0, h->shortest.d_cost.p, (size_t)c * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(h->shortest.rounds.data() + q0, h->shortest.d_rounds.p, (size_t)c * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(h->shortest.relaxed.data() + q0, h->shortest.d_relaxed.p, (size_t)c * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(clk.mark(kResultsEnd, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->batch.ms[0] += clk.ms(kRoundBegin, kFlagsEnd);
    h->batch.ms[1] += clk.ms(kFlagsEnd, kSearchEnd);
    h->batch.ms[3] += clk.ms(kSearchEnd, kResultsEnd);
    if (br.mode < 0) return OXHIP_OK;
    h->shortest.ms[2] += clk.ms(kFlagsEnd, kLabelsEnd);
    h->shortest.ms[3] += clk.ms(kLabelsEnd, kSearchEnd);
    for (uint32_t i = 0; i < c; ++i)
        if ((int32_t)br.res[i] == OXHIP_ERR_HIP)   // (no query status is OXHIP_ERR_HIP otherwise)
            return fail(OXHIP_ERR_HIP, "shortest-path search: a label round or level cap was hit, which cannot happen");
    return OXHIP_OK;
}

// the round's results into the per-query vectors; returns the rows of the round's paths (br.off: where each begins among them)
uint64_t scatter_round(oxhip_prm* h, BatchRun& br, uint32_t q0, uint32_t c) {
    const size_t chunk = br.chunk;
    uint64_t rows = 0;
    const uint64_t row0 = h->batch.off[q0];
    for (uint32_t i = 0; i < c; ++i) {
        h->batch.status[q0 + i] = (int32_t)br.res[i];
        h->batch.len[q0 + i] = br.res[chunk + i];
        h->batch.goal_node[q0 + i] = (int32_t)br.res[2 * chunk + i];
        h->batch.nstart[q0 + i] = br.res[3 * chunk + i];
        h->batch.ngoal[q0 + i] = br.res[4 * chunk + i];
        br.off[i] = rows;
        rows += br.res[chunk + i];
        h->batch.off[q0 + i + 1] = row0 + rows;
    }
    return rows;
}

// the `rows` path rows of the round, extracted on the device and appended to batch.nodes / batch.rows
int32_t extract_round_paths(oxhip_prm* h, const BatchRun& br, const PrmBatchArgs& b, uint64_t rows) {
    const uint32_t dim = h->cfg.dim;
    const uint64_t row0 = h->batch.off[b.q0];
    HIP_TRY(h->batch.d_nodes.reserve((size_t)rows)); HIP_TRY(h->batch.d_rows.reserve((size_t)rows * dim));
    h->batch.nodes.resize((size_t)(row0 + rows)); h->batch.rows.resize((size_t)(row0 + rows) * dim);
    HIP_TRY(hipMemcpyAsync(h->batch.d_off.p, br.off.data(), (size_t)b.n_chunk * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h->batch.clk.mark(kPathsBegin, h->stream));
    launch_prm_batch_paths(b, h->batch.d_off.p, h->batch.d_nodes.p, h->batch.d_rows.p, h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(h->batch.clk.mark(kPathsEnd, h->stream));
    HIP_TRY(hipMemcpyAsync(h->batch.nodes.data() + row0, h->batch.d_nodes.p, (size_t)rows * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(h->batch.rows.data() + (size_t)row0 * dim, h->batch.d_rows.p, (size_t)rows * dim * sizeof(double), hipMemcpyDeviceToHost,
                           h->stream));
    HIP_TRY(h->batch.clk.mark(kRowsEnd, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->batch.ms[2] += h->batch.clk.ms(kPathsBegin, kPathsEnd);
    h->batch.ms[3] += h->batch.clk.ms(kPathsEnd, kRowsEnd);
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
            ++h->batch.rounds;
            answered = q0 + c;
        }
        for (uint32_t q = answered + 1; q <= br.Q; ++q) h->batch.off[q] = h->batch.off[answered];   // (the rounds not begun add no rows)
    }
    if (mode >= 0) { h->shortest.ms[1] = h->batch.ms[0]; h->shortest.ms[4] = h->batch.ms[2]; h->shortest.ms[5] = h->batch.ms[3]; }
    h->batch.valid = true;
    if (status_out) for (uint32_t q = 0; q < br.Q; ++q) status_out[q] = h->batch.status[q];
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
    if (!h->batch.valid) return fail(OXHIP_ERR_UNSAMPLED_STATE_SPACE, "no batch was solved on this roadmap");
    if (h->batch.mode < 0) return fail(OXHIP_ERR_BAD_ARG, "the last batch was not a shortest-path batch");
    if (cost && !h->shortest.cost.empty()) std::memcpy(cost, h->shortest.cost.data(), h->shortest.cost.size() * sizeof(double));
    return OXHIP_OK;
}

int32_t oxhip_prm_batch_get_labels(oxhip_prm* h, uint32_t query, double* cost, uint32_t* hops, uint32_t* parent, uint32_t cap) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (!h->batch.valid) return fail(OXHIP_ERR_UNSAMPLED_STATE_SPACE, "no batch was solved on this roadmap");
    if (h->batch.mode < 0) return fail(OXHIP_ERR_BAD_ARG, "the last batch was not a shortest-path batch");
    if (query >= h->batch.status.size()) return fail(OXHIP_ERR_BAD_ARG, "query index beyond the last batch");
    const uint32_t n = h->rm.n;
    if ((cost || hops || parent) && cap < n) return fail(OXHIP_ERR_CAPACITY, "label buffers too small");
    if (!cost && !hops && !parent) return OXHIP_OK;
    if (h->batch.status[query] == OXHIP_ERR_INVALID_START_STATE || h->batch.status[query] == OXHIP_ERR_TIMEOUT) {   // no search ran
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
    const PrmBatchArgs b = batch_args(h, query, 1, (uint32_t)(h->batch.d_res.n / 5));
    const PrmShortestArgs sa = shortest_args(h, h->batch.mode);
    const uint32_t group = prm_batch_group(n, h->rm.n_keys);
    OX_TRY(launch_shortest(h, b, sa, group, false));
    int32_t status = 0;
    HIP_TRY(hipMemcpyAsync(&status, h->batch.d_res.p, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (cost) HIP_TRY(hipMemcpyAsync(cost, h->shortest.d_label.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (hops) HIP_TRY(hipMemcpyAsync(hops, h->shortest.d_stamp.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    if (parent) HIP_TRY(hipMemcpyAsync(parent, h->batch.d_parent.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (status == OXHIP_ERR_HIP) return fail(OXHIP_ERR_HIP, "shortest-path search: a label round or level cap was hit, which cannot happen");
    return OXHIP_OK;
}

int32_t oxhip_prm_batch_get_search_stats(oxhip_prm* h, uint32_t* label_rounds, uint64_t* relaxations, double* phase_ms) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (!h->batch.valid) return fail(OXHIP_ERR_UNSAMPLED_STATE_SPACE, "no batch was solved on this roadmap");
    if (h->batch.mode < 0) return fail(OXHIP_ERR_BAD_ARG, "the last batch was not a shortest-path batch");
    const size_t Q = h->shortest.rounds.size();
    if (label_rounds && Q) std::memcpy(label_rounds, h->shortest.rounds.data(), Q * sizeof(uint32_t));
    if (relaxations && Q) std::memcpy(relaxations, h->shortest.relaxed.data(), Q * sizeof(uint64_t));
    if (phase_ms) for (int i = 0; i < 6; ++i) phase_ms[i] = h->shortest.ms[i];
    return OXHIP_OK;
}

int32_t oxhip_prm_batch_get_results(oxhip_prm* h, int32_t* status, uint32_t* path_len, int32_t* goal_node, uint32_t* n_start, uint32_t* n_goal) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (!h->batch.valid) return fail(OXHIP_ERR_UNSAMPLED_STATE_SPACE, "no batch was solved on this roadmap");
    const size_t Q = h->batch.status.size();
    if (status && Q) std::memcpy(status, h->batch.status.data(), Q * sizeof(int32_t));
    if (path_len && Q) std::memcpy(path_len, h->batch.len.data(), Q * sizeof(uint32_t));
    if (goal_node && Q) std::memcpy(goal_node, h->batch.goal_node.data(), Q * sizeof(int32_t));
    if (n_start && Q) std::memcpy(n_start, h->batch.nstart.data(), Q * sizeof(uint32_t));
    if (n_goal && Q) std::memcpy(n_goal, h->batch.ngoal.data(), Q * sizeof(uint32_t));
    return OXHIP_OK;
}

int32_t oxhip_prm_batch_get_paths(oxhip_prm* h, uint64_t* offsets, uint32_t* nodes, double* states, uint64_t cap_rows, uint64_t* total_rows) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (!h->batch.valid) return fail(OXHIP_ERR_UNSAMPLED_STATE_SPACE, "no batch was solved on this roadmap");
    const uint64_t total = h->batch.nodes.size();
    if (total_rows) *total_rows = total;
    if (offsets) std::memcpy(offsets, h->batch.off.data(), h->batch.off.size() * sizeof(uint64_t));
    if ((nodes || states) && cap_rows < total) return fail(OXHIP_ERR_CAPACITY, "path buffers too small");
    if (nodes && total) std::memcpy(nodes, h->batch.nodes.data(), (size_t)total * sizeof(uint32_t));
    if (states && total) std::memcpy(states, h->batch.rows.data(), h->batch.rows.size() * sizeof(double));
    return OXHIP_OK;
}

int32_t oxhip_prm_batch_get_query_sets(oxhip_prm* h, uint32_t query, uint32_t* start_connections, uint32_t cap_start, uint32_t* n_start,
                                       uint32_t* goal_indices, uint32_t cap_goal, uint32_t* n_goal) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (!h->batch.valid) return fail(OXHIP_ERR_UNSAMPLED_STATE_SPACE, "no batch was solved on this roadmap");
    if (query >= h->batch.status.size()) return fail(OXHIP_ERR_BAD_ARG, "query index beyond the last batch");
    const uint32_t ns = h->batch.nstart[query], ng = h->batch.ngoal[query];
    if (n_start) *n_start = ns;
    if (n_goal) *n_goal = ng;
    if (start_connections && cap_start < ns) return fail(OXHIP_ERR_CAPACITY, "start_connections buffer too small");
    if (goal_indices && cap_goal < ng) return fail(OXHIP_ERR_CAPACITY, "goal_indices buffer too small");
    if ((!start_connections && !goal_indices) || (ns == 0 && ng == 0)) return OXHIP_OK;
    // the sets are not kept per query: the flag kernel runs again for this one (same kernel, same bits) into workspace row 0
    OX_TRY(select_device(h->cfg.device));
    const uint32_t n = h->rm.n;
    const PrmBatchArgs b = batch_args(h, query, 1, (uint32_t)(h->batch.d_res.n / 5));
    launch_batch_flags(h, b);
    HIP_TRY(hipGetLastError());
    std::vector<uint8_t> flags(n);
    HIP_TRY(hipMemcpyAsync(flags.data(), h->batch.d_flags.p, n, hipMemcpyDeviceToHost, h->stream));
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
    if (phase_ms) for (int i = 0; i < 4; ++i) phase_ms[i] = h->batch.ms[i];
    if (rounds) *rounds = h->batch.rounds;
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

// "Is every milestone valid now": is_valid(milestone i) under the obstacles as they are, by the re-check's kernel, into reval.valid;
// reval.counters[kRevalInvalid] counts the zeros.  clk (or null): bracket the kernel with the marks begin, begin + 1.  n_invalid
// (or null): read the count back, which synchronises the stream.  The re-check, growth's liveness mask and prune's stage 1 start here.
int32_t milestone_validity(oxhip_prm* h, PhaseClock* clk, int begin, uint32_t* n_invalid) {
    HIP_TRY(h->reval.valid.reserve(h->rm.n)); HIP_TRY(h->reval.counters.reserve(kRevalCounters));   // (hipMalloc blocks: reserve_prune has done it)
    HIP_TRY(hipMemsetAsync(h->reval.counters.p, 0, kRevalCounters * sizeof(uint32_t), h->stream));
    if (clk) HIP_TRY(clk->mark(begin, h->stream));
    launch_prm_reval_valid(h->so3, h->dp, h->rm.ms.p, h->rm.n, h->reval.valid.p, h->reval.counters.p, h->stream);
    HIP_TRY(hipGetLastError());
    if (clk) HIP_TRY(clk->mark(begin + 1, h->stream));
    if (!n_invalid) return OXHIP_OK;
    HIP_TRY(hipMemcpyAsync(n_invalid, h->reval.counters.p + kRevalInvalid, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
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
    HIP_TRY(hipMemcpyAsync(h->rm.ms.p, s_ms.p, (size_t)n * dim * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->rm.offsets.p, s_off.p, ((size_t)n + 1) * sizeof(uint32_t), hipMemcpyDeviceToDevice, h->stream));
    launch_planted_shadow(h, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->rm.nbrs.swap(s_nbrs);
    bind_roadmap(h);
    clear_roadmap(h, n, n_entries);   // everything that belonged to the roadmap before; n_samples = redraw_batches = 0
    return OXHIP_OK;
}

int32_t oxhip_prm_revalidate(oxhip_prm* h, uint8_t* milestone_valid, uint32_t* n_invalid_milestones, uint64_t* n_removed_entries) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (!h->is_setup) return fail(OXHIP_ERR_PLANNER_UNINITIALISED, "setup() was not called");
    if (h->rm.n == 0) return fail(OXHIP_ERR_UNSAMPLED_STATE_SPACE, "the roadmap holds no milestones");
    OX_TRY(select_device(h->cfg.device));
    const uint32_t n = h->rm.n, n_old = h->rm.n_keys, pair_cap = n_old / 2 + 1;
    // every buffer before the timed region: hipMalloc is a blocking call
    size_t tmp_bytes = 0;
    if (n_old) {
        HIP_TRY(h->reval.keep.reserve(n_old)); HIP_TRY(h->reval.pos.reserve(n_old)); HIP_TRY(h->reval.nbrs.reserve(n_old));
        OX_TRY(reserve_reval_pairs(h, pair_cap));
        HIP_TRY(prm_reval_scan(nullptr, tmp_bytes, h->reval.keep.p, h->reval.pos.p, n_old, h->stream));
        HIP_TRY(h->reval.tmp.reserve(tmp_bytes));
    }
    PhaseClock& clk = h->reval.clk;
    uint32_t cnt[kRevalCounters] = {};
    if (n_old) HIP_TRY(hipMemsetAsync(h->reval.keep.p, 0, n_old, h->stream));
    OX_TRY(milestone_validity(h, &clk, kRvBegin, nullptr));   // kRvBegin, kRvValidEnd
    launch_prm_reval_emit(h->rm.offsets.p, h->rm.nbrs.p, h->reval.valid.p, n, n_old, h->reval.pairs.p, reval_cand(h), pair_cap,
                          h->reval.counters.p, h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(clk.mark(kRvEmitEnd, h->stream));
    HIP_TRY(hipMemcpyAsync(cnt, h->reval.counters.p, sizeof cnt, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (cnt[kRevalPairs] > pair_cap) return fail(OXHIP_ERR_HIP, "revalidate: more lower-index entries than half the roadmap's, which a symmetric roadmap cannot have");
    HIP_TRY(clk.mark(kRvEdgesBegin, h->stream));
    OX_TRY(launch_reval_edges(h, cnt[kRevalPairs], n, n_old));
    HIP_TRY(hipGetLastError());
    HIP_TRY(clk.mark(kRvEdgesEnd, h->stream));
    uint32_t n_new = 0;
    if (n_old) {
        HIP_TRY(prm_reval_scan(h->reval.tmp.p, tmp_bytes, h->reval.keep.p, h->reval.pos.p, n_old, h->stream));
        launch_prm_reval_compact(h->rm.offsets.p, h->rm.nbrs.p, h->reval.keep.p, h->reval.pos.p, n, n_old, h->reval.nbrs.p, h->stream);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(clk.mark(kRvCompactEnd, h->stream));
    if (n_old) HIP_TRY(hipMemcpyAsync(&n_new, h->rm.offsets.p + n, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    if (milestone_valid) HIP_TRY(hipMemcpyAsync(milestone_valid, h->reval.valid.p, n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->reval.ms[0] = clk.ms(kRvBegin, kRvValidEnd);
    h->reval.ms[1] = clk.ms(kRvValidEnd, kRvEmitEnd);
    h->reval.ms[2] = clk.ms(kRvEdgesBegin, kRvEdgesEnd);
    h->reval.ms[3] = clk.ms(kRvEdgesEnd, kRvCompactEnd);
    if (n_old) h->rm.nbrs.swap(h->reval.nbrs);
    bind_roadmap(h);
    h->rm.n_keys = n_new;
    drop_derived(h);   // the host copy (the single solve searches it), the last solve's sets, the last batch, the edge weights
    if (n_invalid_milestones) *n_invalid_milestones = cnt[kRevalInvalid];
    if (n_removed_entries) *n_removed_entries = (uint64_t)n_old - n_new;
    return OXHIP_OK;
}

int32_t oxhip_prm_revalidate_last_timing(oxhip_prm* h, double* phase_ms) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (phase_ms) for (int i = 0; i < 4; ++i) phase_ms[i] = h->reval.ms[i];
    return OXHIP_OK;
}

}  // extern "C"

// ---- a roadmap grown in place: oxhip_prm_grow_roadmap in its steps

namespace {

// every buffer alloc_prm sizes by the capacity, moved to `cap` with the roadmap's part of its contents (the query flags hold
// nothing between calls)
int32_t grow_capacity(oxhip_prm* h, uint32_t cap) {
    const size_t dim = h->cfg.dim, n = h->rm.n;
    DevBuf<double> ms;
    DevBuf<float> ms32;
    DevBuf<uint8_t> flags;
    DevBuf<uint32_t> offsets;
    HIP_TRY(ms.alloc(dim * cap)); HIP_TRY(flags.alloc(cap)); HIP_TRY(offsets.alloc((size_t)cap + 1));
    if (!h->so3) HIP_TRY(ms32.alloc(dim * cap));
    HIP_TRY(hipMemcpyAsync(ms.p, h->rm.ms.p, n * dim * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    if (!h->so3) HIP_TRY(hipMemcpyAsync(ms32.p, h->rm.ms32.p, n * dim * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(offsets.p, h->rm.offsets.p, (n + 1) * sizeof(uint32_t), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->rm.ms.swap(ms); h->rm.ms32.swap(ms32); h->rm.offsets.swap(offsets); h->single.flags.swap(flags);
    h->args.cap = cap;
    bind_roadmap(h);
    return OXHIP_OK;
}

// the directed keys of the roadmap as it stands, under the current capacity's shift: what this call's edge keys are appended to
int32_t keys_from_csr(oxhip_prm* h) {
    HIP_TRY(h->work.keys.reserve(std::max<size_t>(h->rm.n_keys, 1)));
    h->args.keys = h->work.keys.p;
    HIP_TRY(h->grow.tally.clk.mark(kBegin, h->stream));
    launch_prm_grow_keys(h->rm.offsets.p, h->rm.nbrs.p, h->rm.n, h->rm.n_keys, prm_key_shift(h->args.cap), h->work.keys.p, h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(h->grow.tally.clk.mark(kEnd, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->grow.keys_ms = h->grow.tally.clk.ms(kBegin, kEnd);
    return OXHIP_OK;
}

// the candidates whose earlier end is live, into grow.cand: `pairs` and st.n_cand come back as what the edge step reads (pairs phase)
int32_t drop_dead_candidates(oxhip_prm* h, PrmState& st, uint32_t n_old, uint2*& pairs) {
    const uint32_t nc = (uint32_t)st.n_cand;
    uint32_t kept = 0;
    HIP_TRY(h->grow.cand.reserve(std::max<uint32_t>(nc, 1))); HIP_TRY(h->grow.count.reserve(1));
    HIP_TRY(hipMemsetAsync(h->grow.count.p, 0, sizeof(uint32_t), h->stream));
    PrmBuildTally& t = h->grow.tally;
    HIP_TRY(t.clk.mark(kBegin, h->stream));
    launch_prm_grow_filter(pairs, nc, h->reval.valid.p, n_old, h->grow.cand.p, h->grow.count.p, h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(t.clk.mark(kEnd, h->stream));
    HIP_TRY(hipMemcpyAsync(&kept, h->grow.count.p, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    t.ms[1] += t.clk.ms(kBegin, kEnd);
    st.n_cand = kept;
    pairs = h->grow.cand.p;
    return OXHIP_OK;
}

// construction's round for the milestones [n_old, n_now) on the roadmap that exists: sample, pairs, edges, sort + CSR
int32_t grow_round(oxhip_prm* h, PrmState& st, uint32_t n_more, uint64_t sample_limit, bool any_dead) {
    const uint32_t n_old = h->rm.n, knn_k = h->cfg.knn_k;
    PrmBuildTally& t = h->grow.tally;
    OX_TRY(write_state(h, st));
    OX_TRY(sample_until(h, t, st, n_old + n_more, sample_limit));
    const uint32_t n_now = st.n_milestones;
    if (n_now > n_old && n_now >= 2 && (h->thr_conn >= 0.0 || knn_k)) {   // (construct_roadmap's condition)
        if (knn_k) OX_TRY(knn_row_radii(h, st, n_old, n_now));
        OX_TRY(find_pairs(h, t, st, n_old, n_now));
        uint2* pairs = h->work.cand.p;
        if (knn_k) OX_TRY(knn_select(h, t, st, n_old, n_now, pairs));
        else if (any_dead) OX_TRY(drop_dead_candidates(h, st, n_old, pairs));   // no dead milestone: exactly construction's candidates
        OX_TRY(reserve_keys(h, st));
        OX_TRY(check_edges(h, t, st, pairs));
    }
    return build_csr(h, t, n_now, st.n_keys);
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
    if (h->rm.n == 0) return fail(OXHIP_ERR_UNSAMPLED_STATE_SPACE, "the roadmap holds no milestones: construct_roadmap() builds one");
    const bool new_stream = (g->flags & OXHIP_PRM_GROW_NEW_STREAM) != 0;
    if (!new_stream && !h->sampler.pos_valid)
        return fail(OXHIP_ERR_BAD_ARG, "this roadmap was not constructed by this handle, so there is no stream position to continue: "
                                       "pass OXHIP_PRM_GROW_NEW_STREAM with a stream id");
    const uint32_t n_old = h->rm.n;
    if ((uint64_t)n_old + g->n_more > (1ull << 26)) return fail(OXHIP_ERR_CAPACITY, "n + n_more exceeds 2^26 milestones");
    OX_TRY(select_device(h->cfg.device));
    uint32_t n_dead = 0;   // the liveness mask: which earlier milestones are valid now, into reval.valid; n_dead = its zeros
    OX_TRY(milestone_validity(h, &h->grow.tally.clk, kBegin, &n_dead));
    h->grow.mask_ms = h->grow.tally.clk.ms(kBegin, kEnd);
    if (h->cfg.knn_k && n_dead)
        return fail(OXHIP_ERR_BAD_ARG, "k-nearest growth over invalid milestones is not built (" + std::to_string(n_dead) + " are invalid now)");
    if (n_old + g->n_more > h->args.cap) {
        uint32_t cap = 1024;   // the next power of two: above alloc_prm's multiple of 1024, at most 2^26
        while (cap < n_old + g->n_more) cap *= 2;
        OX_TRY(grow_capacity(h, cap));
    }
    OX_TRY(keys_from_csr(h));
    h->grow.tally.reset();   // (after the mask and the keys, which only borrow its clock)
    const uint64_t budget = g->max_samples ? g->max_samples : 4096ull * g->n_more + (1ull << 22);
    const uint64_t sample_limit = budget > ~0ull - h->sampler.n_samples ? ~0ull : h->sampler.n_samples + budget;
    PrmState st{};
    st.draws = new_stream ? 0 : h->sampler.pos_draws;
    st.n_samples = h->sampler.n_samples;
    st.n_milestones = n_old;
    st.n_keys = h->rm.n_keys;
    st.redraw_batches = h->sampler.redraw_batches;
    h->args.stream = new_stream ? g->stream : h->sampler.pos_stream;
    const int32_t status = grow_round(h, st, g->n_more, sample_limit, n_dead != 0);
    const uint64_t stream_used = h->args.stream;
    h->args.stream = h->cfg.stream;   // construct_roadmap after a setup() draws from the configured stream
    // oxhip_prm_last_timing's candidates and oxhip_prm_knn_exact_rows count the roadmap's, not a call's: a grow adds its own to
    // construction's, whether it succeeds or not (tests/test_gpu_prm_timing_contract.py); the phase times stay each call's own
    h->built.candidates += h->grow.tally.candidates; h->built.exact_rows += h->grow.tally.exact_rows;
    if (status != OXHIP_OK) return status;
    *n_added = st.n_milestones - n_old;
    *n_samples_drawn = st.n_samples - h->sampler.n_samples;
    h->rm.n = st.n_milestones;
    h->rm.n_keys = st.n_keys;
    h->sampler.n_samples = st.n_samples;
    h->sampler.redraw_batches = st.redraw_batches;
    h->sampler.pos_valid = true; h->sampler.pos_stream = stream_used; h->sampler.pos_draws = st.draws;
    drop_derived(h);   // the host copy, the last solve's sets, the last batch, the edge weights
    return OXHIP_OK;
}

int32_t oxhip_prm_grow_last_timing(oxhip_prm* h, double* phase_ms) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (phase_ms) for (int i = 0; i < 6; ++i) phase_ms[i] = i == 0 ? h->grow.mask_ms : i == 1 ? h->grow.keys_ms : h->grow.tally.ms[i - 2];
    return OXHIP_OK;
}

}  // extern "C"

// ---- the roadmap as a graph: its connected components, and the roadmap pruned

namespace {

PrmCcBuffers cc_buffers(oxhip_prm* h) { return PrmCcBuffers{h->cc.parent.p, h->cc.label.p, h->cc.count.p, h->cc.size.p, h->cc.summary.p}; }

// the union-find's arrays for the roadmap as it stands: before any timed region (hipMalloc is a blocking call)
int32_t reserve_components(oxhip_prm* h) {
    const size_t n = h->rm.n;
    HIP_TRY(h->cc.parent.reserve(n)); HIP_TRY(h->cc.label.reserve(n)); HIP_TRY(h->cc.count.reserve(n)); HIP_TRY(h->cc.size.reserve(n));
    HIP_TRY(h->cc.summary.reserve(kCcSummaryWords));
    return OXHIP_OK;
}

// labels, sizes and summary of the CSR into cc's buffers; alive (device, [n], or null): prune's stage-1 survivors.  Marks the caller's
// clock around its three phases: first (begin), + 1 (hooked), + 2 (flat), + 3 (end); the kept labels are the whole roadmap's only without a mask.
int32_t components_of(oxhip_prm* h, const uint8_t* alive, PhaseClock& clk, int first) {
    h->cc.valid = false;
    HIP_TRY(clk.mark(first, h->stream));
    launch_prm_components(h->rm.offsets.p, h->rm.nbrs.p, alive, h->rm.n, h->rm.n_keys, cc_buffers(h), clk.event(first + 1), clk.event(first + 2), h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(clk.mark(first + 3, h->stream));
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
    const size_t n = h->rm.n, ne = h->rm.n_keys, dim = h->cfg.dim, cap = h->args.cap;
    HIP_TRY(h->prune.keep.reserve(n)); HIP_TRY(h->prune.pos.reserve(n)); HIP_TRY(h->prune.index.reserve(n)); HIP_TRY(h->prune.kept.reserve(2));
    if (flags & OXHIP_PRM_PRUNE_MASK) HIP_TRY(h->prune.mask.reserve(n));
    if (flags & OXHIP_PRM_PRUNE_INVALID) { HIP_TRY(h->reval.valid.reserve(n)); HIP_TRY(h->reval.counters.reserve(kRevalCounters)); }   // (milestone_validity's)
    if (flags & (OXHIP_PRM_PRUNE_MIN_SIZE | OXHIP_PRM_PRUNE_LARGEST)) OX_TRY(reserve_components(h));
    HIP_TRY(h->prune.ekeep.reserve(std::max<size_t>(ne, 1))); HIP_TRY(h->prune.epos.reserve(std::max<size_t>(ne, 1)));
    HIP_TRY(h->spare.nbrs.reserve(std::max<size_t>(ne, 1)));
    if (h->spare.offsets.n != cap + 1) HIP_TRY(h->spare.offsets.alloc(cap + 1));   // swapped with offsets: the capacity's size exactly
    if (h->spare.ms.n != dim * cap) HIP_TRY(h->spare.ms.alloc(dim * cap));
    if (!h->so3 && h->spare.ms32.n != dim * cap) HIP_TRY(h->spare.ms32.alloc(dim * cap));
    size_t a = 0, b = 0;
    HIP_TRY(prm_reval_scan(nullptr, a, h->prune.keep.p, h->prune.pos.p, (uint32_t)n, h->stream));
    if (ne) HIP_TRY(prm_reval_scan(nullptr, b, h->prune.ekeep.p, h->prune.epos.p, (uint32_t)ne, h->stream));
    tmp_bytes = std::max(a, b);
    HIP_TRY(h->reval.tmp.reserve(tmp_bytes));
    return OXHIP_OK;
}

// stage 1 into prune.keep: INVALID by milestone_validity (no mark, no read-back: nothing waits inside the masks phase), MASK from prune.mask
int32_t prune_stage1_mask(oxhip_prm* h, uint32_t flags) {
    const uint8_t *valid = nullptr, *mask = nullptr;
    if (flags & OXHIP_PRM_PRUNE_INVALID) {
        OX_TRY(milestone_validity(h, nullptr, 0, nullptr));
        valid = h->reval.valid.p;
    }
    if (flags & OXHIP_PRM_PRUNE_MASK) mask = h->prune.mask.p;
    launch_prm_prune_stage1(valid, mask, h->rm.n, h->prune.keep.p, h->prune.kept.p, h->stream);
    HIP_TRY(hipGetLastError());
    return OXHIP_OK;
}

// stage 2 on the components of the stage-1 survivors (cc's buffers): MIN_SIZE and LARGEST into prune.keep
int32_t prune_stage2_mask(oxhip_prm* h, const oxhip_prm_prune_config* c) {
    launch_prm_prune_stage2(cc_buffers(h), h->rm.n, (c->flags & OXHIP_PRM_PRUNE_MIN_SIZE) ? c->min_size : 0u,
                            (c->flags & OXHIP_PRM_PRUNE_LARGEST) != 0, h->prune.keep.p, h->prune.kept.p + 1, h->stream);
    HIP_TRY(hipGetLastError());
    return OXHIP_OK;
}

// the roadmap of the n_kept milestones of prune.keep, into the spare roadmap's buffers; the handle takes them when everything has run
int32_t compact_roadmap(oxhip_prm* h, uint32_t n_kept, size_t tmp_bytes, int32_t* new_index, uint32_t& n_entries_new) {
    const uint32_t n = h->rm.n, ne = h->rm.n_keys, dim = h->cfg.dim;
    PhaseClock& clk = h->prune.clk;
    HIP_TRY(clk.mark(kPrScanBegin, h->stream));
    HIP_TRY(prm_reval_scan(h->reval.tmp.p, tmp_bytes, h->prune.keep.p, h->prune.pos.p, n, h->stream));
    launch_prm_prune_flags(h->rm.offsets.p, h->rm.nbrs.p, h->prune.keep.p, h->prune.pos.p, n, ne, h->prune.index.p, h->prune.ekeep.p, h->stream);
    HIP_TRY(hipGetLastError());
    if (ne) HIP_TRY(prm_reval_scan(h->reval.tmp.p, tmp_bytes, h->prune.ekeep.p, h->prune.epos.p, ne, h->stream));
    HIP_TRY(clk.mark(kPrScanEnd, h->stream));
    if (ne) launch_prm_prune_entries(h->rm.offsets.p, h->rm.nbrs.p, h->prune.ekeep.p, h->prune.epos.p, h->prune.index.p, n, ne, n_kept, h->spare.offsets.p,
                                     h->spare.nbrs.p, h->stream);
    else HIP_TRY(hipMemsetAsync(h->spare.offsets.p, 0, ((size_t)n_kept + 1) * sizeof(uint32_t), h->stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(clk.mark(kPrEntriesEnd, h->stream));
    launch_prm_prune_states(h->rm.ms.p, h->so3 ? nullptr : h->rm.ms32.p, h->prune.index.p, n, dim, h->spare.ms.p, h->so3 ? nullptr : h->spare.ms32.p, h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(clk.mark(kPrStatesEnd, h->stream));
    n_entries_new = 0;
    if (ne) HIP_TRY(hipMemcpyAsync(&n_entries_new, h->spare.offsets.p + n_kept, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    if (new_index) HIP_TRY(hipMemcpyAsync(new_index, h->prune.index.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->rm.offsets.swap(h->spare.offsets); h->rm.nbrs.swap(h->spare.nbrs); h->rm.ms.swap(h->spare.ms);
    if (!h->so3) h->rm.ms32.swap(h->spare.ms32);
    bind_roadmap(h);
    return OXHIP_OK;
}

}  // namespace

extern "C" {

int32_t oxhip_prm_components(oxhip_prm* h, uint32_t* label, uint32_t* size, uint32_t cap, uint32_t* n_components, uint32_t* largest_label,
                             uint32_t* largest_size) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (!h->is_setup) return fail(OXHIP_ERR_PLANNER_UNINITIALISED, "setup() was not called");
    if (h->rm.n == 0) return fail(OXHIP_ERR_UNSAMPLED_STATE_SPACE, "the roadmap holds no milestones");
    if ((label || size) && cap < h->rm.n) return fail(OXHIP_ERR_CAPACITY, "label / size buffers too small");
    OX_TRY(select_device(h->cfg.device));
    const uint32_t n = h->rm.n;
    const bool compute = !h->cc.valid;
    if (compute) {
        OX_TRY(reserve_components(h));
        OX_TRY(components_of(h, nullptr, h->cc.clk, kCcBegin));
    }
    unsigned long long summary[kCcSummaryWords] = {};
    HIP_TRY(h->cc.clk.mark(kCcCopyBegin, h->stream));
    HIP_TRY(hipMemcpyAsync(summary, h->cc.summary.p, sizeof summary, hipMemcpyDeviceToHost, h->stream));
    if (label) HIP_TRY(hipMemcpyAsync(label, h->cc.label.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    if (size) HIP_TRY(hipMemcpyAsync(size, h->cc.size.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h->cc.clk.mark(kCcCopyEnd, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->cc.ms[0] = compute ? h->cc.clk.ms(kCcBegin, kCcHooked) : 0.0;
    h->cc.ms[1] = compute ? h->cc.clk.ms(kCcHooked, kCcFlat) : 0.0;
    h->cc.ms[2] = compute ? h->cc.clk.ms(kCcFlat, kCcEnd) : 0.0;
    h->cc.ms[3] = h->cc.clk.ms(kCcCopyBegin, kCcCopyEnd);
    h->cc.valid = true;
    if (n_components) *n_components = (uint32_t)summary[kCcRoots];
    if (largest_label) *largest_label = 0xFFFFFFFFu - (uint32_t)summary[kCcBest];
    if (largest_size) *largest_size = (uint32_t)(summary[kCcBest] >> 32);
    return OXHIP_OK;
}

int32_t oxhip_prm_components_last_timing(oxhip_prm* h, double* phase_ms, uint32_t* launches) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (phase_ms) for (int i = 0; i < 4; ++i) phase_ms[i] = h->cc.ms[i];
    if (launches) *launches = kCcLaunches;
    return OXHIP_OK;
}

int32_t oxhip_prm_prune(oxhip_prm* h, const oxhip_prm_prune_config* c, const uint8_t* keep, int32_t* new_index, uint32_t* n_kept,
                        uint64_t* n_removed_entries) {
    OX_TRY(validate_prune_args(h, c, keep));
    if (!h->is_setup) return fail(OXHIP_ERR_PLANNER_UNINITIALISED, "setup() was not called");
    if (h->rm.n == 0) return fail(OXHIP_ERR_UNSAMPLED_STATE_SPACE, "the roadmap holds no milestones");
    OX_TRY(select_device(h->cfg.device));
    const uint32_t n = h->rm.n, n_old = h->rm.n_keys;
    const bool stage2 = (c->flags & (OXHIP_PRM_PRUNE_MIN_SIZE | OXHIP_PRM_PRUNE_LARGEST)) != 0;
    size_t tmp_bytes = 0;
    OX_TRY(reserve_prune(h, c->flags, tmp_bytes));
    if (c->flags & OXHIP_PRM_PRUNE_MASK) HIP_TRY(hipMemcpyAsync(h->prune.mask.p, keep, n, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(h->prune.kept.p, 0, 2 * sizeof(uint32_t), h->stream));
    PhaseClock& clk = h->prune.clk;
    HIP_TRY(clk.mark(kPrBegin, h->stream));
    OX_TRY(prune_stage1_mask(h, c->flags));
    if (stage2) {   // (the labels of the stage-1 survivors are not the roadmap's: components_of forgets the kept ones)
        OX_TRY(components_of(h, h->prune.keep.p, clk, kPrCcBegin));
        OX_TRY(prune_stage2_mask(h, c));
    }
    HIP_TRY(clk.mark(kPrMasksEnd, h->stream));
    uint32_t kept[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(kept, h->prune.kept.p, sizeof kept, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const uint32_t n_new = stage2 ? kept[1] : kept[0];
    if (n_new == 0) return fail(OXHIP_ERR_BAD_ARG, "would keep no milestone");   // only workspace was written so far
    uint32_t n_entries_new = 0;
    OX_TRY(compact_roadmap(h, n_new, tmp_bytes, new_index, n_entries_new));
    // masks = begin -> components begin, plus components end -> masks end; components = the union-find's three phases
    h->prune.ms[0] = stage2 ? clk.ms(kPrBegin, kPrCcBegin) + clk.ms(kPrCcEnd, kPrMasksEnd) : clk.ms(kPrBegin, kPrMasksEnd);
    h->prune.ms[1] = stage2 ? clk.ms(kPrCcBegin, kPrCcEnd) : 0.0;
    h->prune.ms[2] = clk.ms(kPrScanBegin, kPrScanEnd);
    h->prune.ms[3] = clk.ms(kPrScanEnd, kPrEntriesEnd);
    h->prune.ms[4] = clk.ms(kPrEntriesEnd, kPrStatesEnd);
    h->rm.n = n_new;
    h->rm.n_keys = n_entries_new;
    drop_derived(h);   // the host copy, the last solve's sets, the last batch, the edge weights, the kept component labels
    if (n_kept) *n_kept = n_new;
    if (n_removed_entries) *n_removed_entries = (uint64_t)n_old - n_entries_new;
    return OXHIP_OK;
}

int32_t oxhip_prm_prune_last_timing(oxhip_prm* h, double* phase_ms) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (phase_ms) for (int i = 0; i < 5; ++i) phase_ms[i] = h->prune.ms[i];
    return OXHIP_OK;
}

}  // extern "C"

// ---- the handle's own validity checker, and the last batch's answered paths subdivided and shortcut

namespace {

enum SimplifyMark { kSpStageBegin, kSpStageEnd, kSpRoundBegin, kSpRowsEnd, kSpPairsEnd, kSpDpEnd, kSpCopyBegin, kSpCopyEnd };

// what every call of this service opens with: the handle, setup(), and -- for the calls that read the last batch -- the batch
int32_t simplify_ready(const oxhip_prm* h, bool needs_batch) {
    if (!h) return fail(OXHIP_ERR_BAD_ARG, "null handle");
    if (!h->is_setup) return fail(OXHIP_ERR_PLANNER_UNINITIALISED, "setup() was not called");
    if (needs_batch && !h->batch.valid) return fail(OXHIP_ERR_UNSAMPLED_STATE_SPACE, "no batch was solved on this roadmap");
    return OXHIP_OK;
}

int32_t check_subdivide(uint32_t subdivide) {
    if (subdivide == 0 || subdivide > 256u) return fail(OXHIP_ERR_BAD_ARG, "subdivide must be in 1..256");
    return OXHIP_OK;
}

int32_t path_too_large() {
    return fail(OXHIP_ERR_CAPACITY, "one path's pair matrix is larger than 1 GiB: pass a max_span or a smaller subdivide");
}

// one simplify while it runs: its shape, its rounds [first[r], first[r + 1]) and a round's tables on the host
struct SimplifyRun {
    uint32_t Q = 0, m = 1, max_span = 0, width = 0;
    std::vector<uint32_t> first;           // the first query of every round, then Q
    uint64_t max_rows = 0, max_words = 0;  // of the largest round
    uint32_t max_chunk = 0;
    std::vector<uint64_t> doff, woff, soff;
    std::vector<uint32_t> simp_len;
};

// a round's three views of the handle's workspaces: the subdivision, the shortcut over the dense rows, the gather
DenseArgs dense_args(oxhip_prm* h, const SimplifyRun& run, uint32_t q0, uint32_t c) {
    DenseArgs a{};
    a.off = h->simplify.d_off.p; a.rows = h->simplify.d_rows.p; a.doff = h->simplify.d_doff.p; a.dense = h->simplify.d_dense.p;
    a.q0 = q0; a.n_chunk = c; a.m = run.m;
    return a;
}

ShortcutArgs shortcut_args(oxhip_prm* h, const SimplifyRun& run, const DenseArgs& d) {
    ShortcutArgs a{};
    a.len = h->simplify.d_len.p + d.q0; a.row_off = d.doff; a.rows = d.dense; a.woff = h->simplify.d_woff.p; a.bits = h->simplify.d_bits.p;
    a.n_words = run.woff[d.n_chunk]; a.n_chunk = d.n_chunk; a.m = run.m; a.max_span = run.max_span;
    a.filt_base = h->dp.filt_abs;
    return a;
}

ShortcutOut shortcut_out(oxhip_prm* h) {
    ShortcutOut o{};
    o.cost = h->simplify.d_cost.p; o.par = h->simplify.d_par.p; o.idx = h->simplify.d_idx.p; o.simp_len = h->simplify.d_simp_len.p;
    o.raw_cost = h->simplify.d_raw.p; o.simp_cost = h->simplify.d_simp.p; o.checks = h->simplify.d_checks.p;
    return o;
}

DenseOut dense_out(oxhip_prm* h) {
    DenseOut o{};
    o.simp_len = h->simplify.d_simp_len.p; o.idx = h->simplify.d_idx.p;
    o.soff = h->simplify.d_soff.p; o.out_idx = h->simplify.d_out_idx.p; o.out_rows = h->simplify.d_out_rows.p;
    return o;
}

// the batch's raw paths, from its host copy off / rows / len, to the device; the host side of the results starts empty
int32_t stage_paths(oxhip_prm* h, const SimplifyRun& run) {
    auto& sp = h->simplify;
    const size_t total = h->batch.nodes.size();
    sp.valid = false; sp.rounds = 0;
    for (double& t : sp.ms) t = 0.0;
    sp.soff.assign((size_t)run.Q + 1, 0); sp.checks.assign(run.Q, 0);
    sp.raw_cost.assign(run.Q, 0.0); sp.simp_cost.assign(run.Q, 0.0);
    sp.idx.clear(); sp.rows.clear();
    if (!run.Q) return OXHIP_OK;
    HIP_TRY(sp.d_off.reserve((size_t)run.Q + 1)); HIP_TRY(sp.d_len.reserve(run.Q)); HIP_TRY(sp.d_rows.reserve(std::max<size_t>(1, total * run.width)));
    HIP_TRY(sp.clk.mark(kSpStageBegin, h->stream));
    HIP_TRY(hipMemcpyAsync(sp.d_off.p, h->batch.off.data(), ((size_t)run.Q + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(sp.d_len.p, h->batch.len.data(), (size_t)run.Q * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    if (total) HIP_TRY(hipMemcpyAsync(sp.d_rows.p, h->batch.rows.data(), total * run.width * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(sp.clk.mark(kSpStageEnd, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    sp.ms[0] += sp.clk.ms(kSpStageBegin, kSpStageEnd);
    return OXHIP_OK;
}

// The rounds (shortcut_rounds: at most 65,535 queries each, fewer with chunk_queries given) and every buffer the largest needs
int32_t reserve_simplify_workspace(oxhip_prm* h, SimplifyRun& run, uint32_t chunk_queries) {
    uint32_t refused = 0;
    if (!shortcut_rounds(h->batch.len.data(), run.Q, run.m, run.max_span, kShortcutMatrixBytes,
                         chunk_queries ? std::min(chunk_queries, 65535u) : 65535u, run.first, refused))
        return path_too_large();
    for (size_t r = 0; r + 1 < run.first.size(); ++r) {
        uint64_t rows = 0, words = 0;
        for (uint32_t q = run.first[r]; q < run.first[r + 1]; ++q) {
            const ShortcutShape s = shortcut_shape(h->batch.len[q], run.m, run.max_span);
            rows += s.rows; words += s.words;
        }
        run.max_rows = std::max(run.max_rows, rows); run.max_words = std::max(run.max_words, words);
        run.max_chunk = std::max(run.max_chunk, run.first[r + 1] - run.first[r]);
    }
    auto& sp = h->simplify;
    const size_t c1 = (size_t)run.max_chunk + 1, nr = std::max<size_t>(1, run.max_rows);
    HIP_TRY(sp.d_doff.reserve(c1)); HIP_TRY(sp.d_woff.reserve(c1)); HIP_TRY(sp.d_soff.reserve(c1));
    HIP_TRY(sp.d_simp_len.reserve(c1)); HIP_TRY(sp.d_raw.reserve(c1)); HIP_TRY(sp.d_simp.reserve(c1)); HIP_TRY(sp.d_checks.reserve(c1));
    HIP_TRY(sp.d_dense.reserve(nr * run.width)); HIP_TRY(sp.d_out_rows.reserve(nr * run.width));
    HIP_TRY(sp.d_cost.reserve(nr)); HIP_TRY(sp.d_par.reserve(nr)); HIP_TRY(sp.d_idx.reserve(nr)); HIP_TRY(sp.d_out_idx.reserve(nr));
    HIP_TRY(sp.d_bits.reserve(std::max<size_t>(1, run.max_words)));
    run.doff.resize(c1); run.woff.resize(c1); run.soff.resize(c1); run.simp_len.resize(c1);
    return OXHIP_OK;
}

// the round's tables (where each query's dense rows and matrix words begin) and its dense paths
int32_t subdivide_round(oxhip_prm* h, SimplifyRun& run, DenseArgs& a) {
    auto& sp = h->simplify;
    const uint32_t c = a.n_chunk;
    run.doff[0] = run.woff[0] = 0;
    for (uint32_t i = 0; i < c; ++i) {
        const ShortcutShape s = shortcut_shape(h->batch.len[a.q0 + i], run.m, run.max_span);
        run.doff[i + 1] = run.doff[i] + s.rows;
        run.woff[i + 1] = run.woff[i] + s.words;
    }
    a.n_rows = run.doff[c];
    HIP_TRY(sp.clk.mark(kSpRoundBegin, h->stream));
    HIP_TRY(hipMemcpyAsync(sp.d_doff.p, run.doff.data(), ((size_t)c + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(sp.d_woff.p, run.woff.data(), ((size_t)c + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    launch_dense_rows(h->so3, h->cfg.dim, a, h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(sp.clk.mark(kSpRowsEnd, h->stream));
    return OXHIP_OK;
}

// check_motion per pair of the round's windows that is not on one edge, against the obstacles as they are now
int32_t pairs_round(oxhip_prm* h, const ShortcutArgs& a) {
    launch_shortcut_pairs(h->dp, a, true, h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(h->simplify.clk.mark(kSpPairsEnd, h->stream));
    return OXHIP_OK;
}

int32_t dp_round(oxhip_prm* h, const ShortcutArgs& a, const ShortcutOut& o) {
    launch_shortcut_dp(h->dp.space, h->cfg.dim, a, o, h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(h->simplify.clk.mark(kSpDpEnd, h->stream));
    return OXHIP_OK;
}

// the round's chains: their lengths, then indices and rows compacted on the device and appended to the host side; the phase times
int32_t collect_round(oxhip_prm* h, SimplifyRun& run, const DenseArgs& a, const DenseOut& o) {
    auto& sp = h->simplify;
    const uint32_t c = a.n_chunk, q0 = a.q0, width = run.width;
    HIP_TRY(sp.clk.mark(kSpCopyBegin, h->stream));
    HIP_TRY(hipMemcpyAsync(run.simp_len.data(), sp.d_simp_len.p, (size_t)c * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    run.soff[0] = 0;
    for (uint32_t i = 0; i < c; ++i) {
        run.soff[i + 1] = run.soff[i] + run.simp_len[i];
        sp.soff[q0 + i + 1] = sp.soff[q0] + run.soff[i + 1];
    }
    const uint64_t n_out = run.soff[c], row0 = sp.soff[q0];
    if (n_out > a.n_rows) return fail(OXHIP_ERR_HIP, "simplify: a chain longer than its dense path, which cannot happen");
    sp.idx.resize((size_t)(row0 + n_out)); sp.rows.resize((size_t)(row0 + n_out) * width);
    HIP_TRY(hipMemcpyAsync(sp.d_soff.p, run.soff.data(), ((size_t)c + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    launch_dense_gather(width, a, o, h->stream);
    HIP_TRY(hipGetLastError());
    if (n_out) {
        HIP_TRY(hipMemcpyAsync(sp.idx.data() + row0, sp.d_out_idx.p, (size_t)n_out * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(sp.rows.data() + (size_t)row0 * width, sp.d_out_rows.p, (size_t)n_out * width * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipMemcpyAsync(sp.raw_cost.data() + q0, sp.d_raw.p, (size_t)c * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(sp.simp_cost.data() + q0, sp.d_simp.p, (size_t)c * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(sp.checks.data() + q0, sp.d_checks.p, (size_t)c * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(sp.clk.mark(kSpCopyEnd, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    sp.ms[0] += sp.clk.ms(kSpRoundBegin, kSpRowsEnd);
    sp.ms[1] += sp.clk.ms(kSpRowsEnd, kSpPairsEnd);
    sp.ms[2] += sp.clk.ms(kSpPairsEnd, kSpDpEnd);
    sp.ms[3] += sp.clk.ms(kSpCopyBegin, kSpCopyEnd);
    return OXHIP_OK;
}

// the handle's StateValidityChecker and check_motion over caller rows: what an RRT batch of the same space launches
template <typename Launch>
int32_t checker_rows(oxhip_prm* h, const double* a, const double* b, uint32_t n, uint8_t* out, Launch&& launch) {
    OX_TRY(simplify_ready(h, false));
    if (!a || !out) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    if (n == 0) return OXHIP_OK;
    OX_TRY(select_device(h->cfg.device));
    DevBuf<double> da, db;
    DevBuf<uint8_t> dout;
    OX_TRY(to_device(da, a, (size_t)n * h->cfg.dim, h->stream));
    if (b) OX_TRY(to_device(db, b, (size_t)n * h->cfg.dim, h->stream));
    HIP_TRY(dout.alloc(n));
    launch(da.p, db.p, dout.p);
    HIP_TRY(hipGetLastError());
    return to_host(out, dout, n, h->stream);
}

}  // namespace

extern "C" {

int32_t oxhip_prm_is_valid(oxhip_prm* h, const double* states, uint32_t n, uint8_t* out) {
    return checker_rows(h, states, nullptr, n, out, [&](const double* s, const double*, uint8_t* o) {
        if (h->so3) launch_so3_is_valid(h->dp, s, n, o, h->stream);
        else launch_is_valid(h->dp, s, n, o, h->stream);
    });
}

int32_t oxhip_prm_check_motion(oxhip_prm* h, const double* from, const double* to, uint32_t n, uint8_t* out) {
    if (h && !to) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    return checker_rows(h, from, to, n, out, [&](const double* f, const double* t, uint8_t* o) {
        if (h->so3) launch_so3_check_motion(h->dp, f, t, n, o, h->stream);
        else launch_check_motion(h->dp, f, t, n, o, h->stream);
    });
}

int32_t oxhip_prm_batch_simplify_paths(oxhip_prm* h, uint32_t subdivide, uint32_t max_span, uint32_t chunk_queries) {
    OX_TRY(simplify_ready(h, true));
    OX_TRY(check_subdivide(subdivide));
    OX_TRY(select_device(h->cfg.device));
    SimplifyRun run;
    run.Q = (uint32_t)h->batch.status.size(); run.m = subdivide; run.max_span = max_span; run.width = h->cfg.dim;
    OX_TRY(reserve_simplify_workspace(h, run, chunk_queries));   // (refuses a path too large before anything is staged: the last results stay)
    OX_TRY(stage_paths(h, run));
    const ShortcutOut o = shortcut_out(h);
    const DenseOut g = dense_out(h);
    for (size_t r = 0; r + 1 < run.first.size(); ++r) {
        DenseArgs d = dense_args(h, run, run.first[r], run.first[r + 1] - run.first[r]);
        OX_TRY(subdivide_round(h, run, d));
        const ShortcutArgs a = shortcut_args(h, run, d);
        OX_TRY(pairs_round(h, a));
        OX_TRY(dp_round(h, a, o));
        OX_TRY(collect_round(h, run, d, g));
        ++h->simplify.rounds;
    }
    h->simplify.valid = true;
    return OXHIP_OK;
}

int32_t oxhip_prm_batch_get_simplified_paths(oxhip_prm* h, uint64_t* offsets, double* states, uint32_t* indices, uint64_t cap_rows,
                                             uint64_t* total_rows) {
    OX_TRY(simplify_ready(h, true));
    if (!h->simplify.valid) return fail(OXHIP_ERR_BAD_ARG, "no simplified paths: call oxhip_prm_batch_simplify_paths after the last batch");
    const uint64_t total = h->simplify.idx.size();
    if (total_rows) *total_rows = total;
    if (offsets) std::memcpy(offsets, h->simplify.soff.data(), h->simplify.soff.size() * sizeof(uint64_t));
    if ((states || indices) && cap_rows < total) return fail(OXHIP_ERR_CAPACITY, "path buffers too small");
    if (indices && total) std::memcpy(indices, h->simplify.idx.data(), (size_t)total * sizeof(uint32_t));
    if (states && total) std::memcpy(states, h->simplify.rows.data(), h->simplify.rows.size() * sizeof(double));
    return OXHIP_OK;
}

int32_t oxhip_prm_batch_get_simplify_results(oxhip_prm* h, double* raw_cost, double* simplified_cost, uint64_t* checks) {
    OX_TRY(simplify_ready(h, true));
    if (!h->simplify.valid) return fail(OXHIP_ERR_BAD_ARG, "no simplified paths: call oxhip_prm_batch_simplify_paths after the last batch");
    const size_t Q = h->simplify.checks.size();
    if (raw_cost && Q) std::memcpy(raw_cost, h->simplify.raw_cost.data(), Q * sizeof(double));
    if (simplified_cost && Q) std::memcpy(simplified_cost, h->simplify.simp_cost.data(), Q * sizeof(double));
    if (checks && Q) std::memcpy(checks, h->simplify.checks.data(), Q * sizeof(uint64_t));
    return OXHIP_OK;
}

// test hook: the pair kernel's verdicts on one query's dense path, in buffers of its own (the last simplify's results stay)
int32_t oxhip_prm_batch_path_valid_matrix(oxhip_prm* h, uint32_t query, uint32_t subdivide, uint32_t max_span, uint8_t* out, uint64_t cap_bytes,
                                          uint32_t* len_out) {
    OX_TRY(simplify_ready(h, true));
    if (!len_out) return fail(OXHIP_ERR_BAD_ARG, "null argument");
    OX_TRY(check_subdivide(subdivide));
    if (query >= h->batch.status.size()) return fail(OXHIP_ERR_BAD_ARG, "query index beyond the last batch");
    const uint32_t L = h->batch.len[query], width = h->cfg.dim, m = subdivide;
    const ShortcutShape sh = shortcut_shape(L, m, max_span);
    const uint64_t M = sh.rows, words = sh.words;
    if (!shortcut_fits(sh, kShortcutMatrixBytes)) return path_too_large();
    *len_out = (uint32_t)M;
    if (!out || M == 0) return OXHIP_OK;
    if (cap_bytes < M * M) return fail(OXHIP_ERR_CAPACITY, "matrix buffer too small");
    OX_TRY(select_device(h->cfg.device));
    const uint64_t off[2] = {0, L}, doff[2] = {0, M}, woff[2] = {0, words};
    DevBuf<uint64_t> d_off, d_doff, d_woff, d_bits;
    DevBuf<uint32_t> d_len;
    DevBuf<double> d_rows, d_dense;
    OX_TRY(to_device(d_off, off, 2, h->stream)); OX_TRY(to_device(d_doff, doff, 2, h->stream)); OX_TRY(to_device(d_woff, woff, 2, h->stream));
    OX_TRY(to_device(d_len, &L, 1, h->stream));
    OX_TRY(to_device(d_rows, h->batch.rows.data() + (size_t)h->batch.off[query] * width, (size_t)L * width, h->stream));
    HIP_TRY(d_dense.alloc((size_t)M * width)); HIP_TRY(d_bits.alloc(std::max<size_t>(1, words)));
    DenseArgs d{};
    d.off = d_off.p; d.rows = d_rows.p; d.doff = d_doff.p; d.dense = d_dense.p; d.n_rows = M; d.q0 = 0; d.n_chunk = 1; d.m = m;
    const ShortcutArgs a{d_len.p, d_doff.p, d_dense.p, d_woff.p, d_bits.p, words, 1, m, max_span, 0, h->dp.filt_abs};
    launch_dense_rows(h->so3, width, d, h->stream);
    launch_shortcut_pairs(h->dp, a, true, h->stream);
    HIP_TRY(hipGetLastError());
    std::vector<uint64_t> bits(words);
    OX_TRY(to_host(bits.data(), d_bits, words, h->stream));
    shortcut_matrix_bytes(bits.data(), L, m, max_span, out);
    return OXHIP_OK;
}

int32_t oxhip_prm_batch_simplify_last_timing(oxhip_prm* h, double* phase_ms, uint32_t* rounds) {
    OX_TRY(simplify_ready(h, false));
    if (phase_ms) for (int i = 0; i < 4; ++i) phase_ms[i] = h->simplify.ms[i];
    if (rounds) *rounds = h->simplify.rounds;
    return OXHIP_OK;
}

}  // extern "C"
