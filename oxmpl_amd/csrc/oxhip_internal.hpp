// oxhip_internal.hpp -- launch wrappers shared between the kernel translation units and the
// C-ABI implementation (oxhip_api.hip).  Not installed; the public surface is include/oxmpl_hip.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace oxhip {

struct DevParams;

// rrt_stream.hip
void launch_rrt_stream(const DevParams& p, hipStream_t stream);
void launch_nn_argmin(uint32_t dim, const double* nodes, const uint64_t* offsets, const uint32_t* n_nodes,
                      uint32_t n_queries, const double* queries, uint32_t* out_index, double* out_min_dist,
                      hipStream_t stream);
void launch_distance(uint32_t dim, const double* a, const double* b, uint32_t n, double* out, hipStream_t s);
void launch_interpolate(uint32_t dim, const double* from, const double* to, const double* t, uint32_t n,
                        double* out, hipStream_t s);
void launch_is_valid(const DevParams& p, const double* states, uint32_t n, uint8_t* out, hipStream_t s);
void launch_check_motion(const DevParams& p, const double* from, const double* to, uint32_t n, uint8_t* out,
                         hipStream_t s);
void launch_f64_op(uint32_t op, const double* a, const double* b, const double* c, uint32_t n, double* out,
                   hipStream_t s);
void launch_rng_u64(uint64_t seed, uint64_t stream, uint32_t n, uint64_t* out, hipStream_t s);

// rrt_connect.hip: RRTConnect (rrt_connect.rs), one 256-thread workgroup per problem, trees streamed from HBM/L2
void launch_rrt_connect(const DevParams& p, hipStream_t stream);

// rrt_connect_se2.hip: RRTConnect over SE(2) among line segments (BASELINE.json configs[3]), one wave per problem
void launch_rrt_connect_se2(const DevParams& p, hipStream_t stream);
uint32_t seg_grid_side();                                                 // cells along an axis of DevParams::seg_grid
void launch_seg_grid(const DevParams& p, uint16_t* grid, double clearance, hipStream_t stream);   // (re)builds it from segs
void launch_se2_op(uint32_t op, const double* a, const double* b, const double* t, uint32_t n, double* out, hipStream_t s);
void launch_se2_is_valid(const DevParams& p, const double* states, uint32_t n, uint8_t* out, hipStream_t s);
void launch_se2_check_motion(const DevParams& p, const double* from, const double* to, uint32_t n, uint8_t* out, hipStream_t s);

// rrt_so2.hip: RRT over SO2StateSpace with the forbidden-arc checker, one wave per problem
void launch_rrt_so2(const DevParams& p, hipStream_t stream);
void launch_so2_is_valid(const DevParams& p, const double* states, uint32_t n, uint8_t* out, hipStream_t s);
void launch_so2_check_motion(const DevParams& p, const double* from, const double* to, uint32_t n, uint8_t* out, hipStream_t s);
// rrt_so3.hip: RRT over SO3StateSpace with the forbidden-cone checker, one wave per problem
void launch_rrt_so3(const DevParams& p, hipStream_t stream);
void launch_so3_op(uint32_t op, const double* a, const double* b, const double* t, uint32_t n, double* out, hipStream_t s);
void launch_so3_is_valid(const DevParams& p, const double* states, uint32_t n, uint8_t* out, hipStream_t s);
void launch_so3_check_motion(const DevParams& p, const double* from, const double* to, uint32_t n, uint8_t* out, hipStream_t s);

// rrt_connect_se3.hip: RRTConnect over SE(3), a rigid body of spheres among sphere obstacles (sph_c [3][n], sph_r), one wave per problem
constexpr int kSe3MaxBody = 16;
struct Se3Args {             // this kernel family's own arguments, next to DevParams
    const double* body;      // [4][kSe3MaxBody] SoA (cx, cy, cz, r) of the body's spheres in the body frame
    uint32_t n_body, pad;
};
void launch_rrt_connect_se3(const DevParams& p, const Se3Args& a, hipStream_t stream);
uint32_t se3_lds_obstacles();                                             // obstacles the kernel stages in LDS (more are read from HBM)
void launch_se3_op(uint32_t op, const double* a, const double* b, const double* t, uint32_t n, double* out, hipStream_t s);
void launch_se3_is_valid(const DevParams& p, const Se3Args& a, const double* states, uint32_t n, uint8_t* out, hipStream_t s);
void launch_se3_check_motion(const DevParams& p, const Se3Args& a, const double* from, const double* to, uint32_t n, uint8_t* out, hipStream_t s);

// rrt_star.hip: RRT* (rrt_star.rs), one 256-thread workgroup per problem
void launch_rrt_star(const DevParams& p, hipStream_t stream);

// rrt_star_wire.hip: the wiring stages of the decoupled RRT* (the geometry comes from launch_rrt_lanes)
bool star_wire_supported(uint32_t dim);
void launch_star_shadow(const DevParams& p, uint32_t max_nodes, hipStream_t stream);   // tree32 and its magnitude bound, nodes [0, n)
void launch_star_count(const DevParams& p, uint32_t max_pending, hipStream_t stream);   // nbr_cnt of the nodes [wired, n)
void launch_star_scan(const DevParams& p, hipStream_t stream);                          // nbr_off, nbr_take
void launch_star_fill(const DevParams& p, uint32_t max_take, hipStream_t stream);       // the lists of [wired, wired + take)
void launch_star_edges(const DevParams& p, uint32_t max_total, hipStream_t stream);     // per pair: distance, both motions' validity
void launch_star_compact(const DevParams& p, uint32_t max_chunks, hipStream_t stream);  // the counting pass's chunks -> the lists (instead of launch_star_fill)
void launch_star_wire(const DevParams& p, hipStream_t stream);                          // choose parent / rewire, node by node

// rrt_resident.hip
// true when a register-resident instantiation exists for (dim, cap)
bool resident_supported(uint32_t dim, uint32_t cap);
void launch_rrt_resident(const DevParams& p, hipStream_t stream);

// rrt_lanes.hip: the resident pipeline with a lane-per-query resolver (64 iterations resolved side by side)
bool lanes_supported(uint32_t dim, uint32_t cap);
void launch_rrt_lanes(const DevParams& p, hipStream_t stream);

// rrt_cells.hip: one wave per problem, nearest neighbour through an exact cell grid (R^2, R^3)
bool cells_supported(uint32_t dim, uint32_t cap);
uint32_t cells_level_max(uint32_t dim, uint32_t cap);
uint32_t cells_head_blocks(uint32_t dim, uint32_t cap);
void launch_rrt_cells(const DevParams& p, hipStream_t stream);
uint32_t sphere_grid_side(uint32_t dim);                                  // cells along an axis of DevParams::sph_grid
void launch_sphere_grid(const DevParams& p, uint64_t* grid, const double* filt, hipStream_t stream);   // (re)builds it from sph_c and the filter thresholds

// prm_kernels.hip: PRM roadmap construction / query (prm.rs)
struct PrmState {            // persists in HBM between launches
    uint64_t draws;          // u64 words consumed from the ChaCha12 stream
    uint64_t n_samples;      // sample_uniform calls made (prm.rs:122)
    unsigned long long n_cand;  // in-radius pairs counted by the current pairs launch (beyond cand_cap: not stored)
    uint32_t n_milestones;   // roadmap.len()
    uint32_t n_keys;         // directed edge keys appended so far (2 per undirected edge)
    uint32_t redraw_batches; // sample batches replayed sequentially because rand rejected a draw
    uint32_t pad;
};
struct PrmArgs {
    double* ms;              // milestones, AoS [cap][dim]
    float* ms32;             // fl32(ms), same layout: what the pair search screens with (its i side is read by scalar loads)
    uint32_t cap;
    uint32_t n_target;       // sample until the roadmap holds this many milestones ...
    uint64_t max_samples;    // ... or this many samples were drawn
    uint64_t stream;         // ChaCha12 stream id (the key is DevParams::seed)
    PrmState* state;
    uint2* cand;             // (j, i) with i < j and distance < connection_radius
    uint32_t cand_cap;
    uint64_t* keys;          // (u << shift) | v for every directed edge u -> v, shift = bits of (cap - 1)
};
struct PrmSpec {              // one round of the parallel sampler
    uint64_t pos0;           // stream word of the round's first sample (= PrmState::draws)
    uint32_t m;              // samples drawn this round
    uint32_t pad;
    double* tmp;             // [m][dim] the round's samples
    uint64_t* vbits;         // [ceil(m/64)] validity ballots
    uint32_t* wave_off;      // [ceil(m/64)] per-wave valid counts, then their exclusive prefix
    uint32_t* redraw_flag;   // set when rand's range sampler would have rejected a draw: the round is replayed
    PrmState* result;        // the state after this round (valid when redraw_flag stays 0)
};
struct PrmQuery {
    double start[8], goal_c[8];
    double goal_thr;         // satisfied iff d2 <= goal_thr
};
void launch_prm_sample(const DevParams& p, const PrmArgs& a, hipStream_t s);
// speculative parallel round: draws, scans, compacts; the host commits sp.result when no draw was rejected
void launch_prm_sample_spec(const DevParams& p, const PrmArgs& a, const PrmSpec& sp, uint32_t n0, hipStream_t s);
// thr_row / thr32_row (optional, [cap]): a threshold per row j instead of `thr` (the k-nearest variant's candidate search)
void launch_prm_pairs(const DevParams& p, const PrmArgs& a, uint32_t j0, uint32_t j1, double thr, hipStream_t s, const double* thr_row = nullptr,
                      const float* thr32_row = nullptr);
float prm_screen_threshold(const DevParams& p, double thr);   // the binary32 screen's threshold for a binary64 d2 threshold
// k-nearest variant: candidates -> sortable keys; sorted keys -> each row's k nearest (`sel`, counters[0] pairs; rows whose radius held
// too few in failed_rows, counters[1] of them); the exact search for those rows
void launch_prm_knn_keys(const PrmArgs& a, uint32_t n_cand, uint64_t* keys, hipStream_t s);
void launch_prm_knn_select(const DevParams& p, const PrmArgs& a, const uint64_t* sorted, double* dist, uint32_t n_sorted, uint32_t j0, uint32_t j1,
                           uint32_t k, uint2* sel, uint32_t* counters, uint32_t* failed_rows, hipStream_t s);
void launch_prm_knn_brute(const DevParams& p, const PrmArgs& a, const uint32_t* failed_rows, uint32_t n_failed, uint32_t k, uint2* sel,
                          uint32_t* counters, hipStream_t s);
void launch_prm_edges(const DevParams& p, const PrmArgs& a, uint32_t n_cand, hipStream_t s);
// rocPRIM radix sort of the directed keys; tmp == nullptr queries tmp_bytes
hipError_t prm_sort_keys(void* tmp, size_t& tmp_bytes, uint64_t* in, uint64_t* out, uint32_t n_keys, uint32_t cap,
                         hipStream_t s);
void launch_prm_csr(const uint64_t* sorted, uint32_t n_keys, uint32_t n_nodes, uint32_t cap, uint32_t* offsets,
                    uint32_t* nbrs, hipStream_t s);
// near: R^n the squared-distance threshold of the connection radius, SO(3) the radius itself (seq_space.hpp: connects)
void launch_prm_query(bool so3, const DevParams& p, const PrmArgs& a, uint32_t n, const PrmQuery& q, double near, uint8_t* flags,
                      uint32_t* start_valid, hipStream_t s);
uint32_t prm_key_shift(uint32_t cap);   // directed keys are (u << shift) | v

// prm_so3.hip: PRM over SO3StateSpace with forbidden cones; the sort / CSR above are shared
struct PrmSo3Spec {           // one round of the SO(3) sampler: m rejection attempts, attempt a at stream word pos0 + 4 a
    uint64_t pos0;
    uint32_t m;
    uint32_t pad;
    double* tmp;             // [m][4] the valid attempts' quaternions
    uint64_t* vbits;         // [ceil(m/64)] ballots of "accepted and valid" (a milestone)
    uint64_t* abits;         // [ceil(m/64)] ballots of "accepted" (a sample_uniform call returned)
    uint32_t* voff;          // [ceil(m/64)] per-wave milestone counts, then their exclusive prefix
    uint32_t* acnt;          // [ceil(m/64)] per-wave sample counts
    uint32_t* redraw_flag;   // set when random_range would have drawn again (unreachable for -1..1): the host refuses the round
    PrmState* result;        // the state after this round
};
void launch_prm_so3_sample(const DevParams& p, const PrmArgs& a, const PrmSo3Spec& sp, uint32_t n0, hipStream_t s);
// candidates (j, i < j) with distance < r, j in [j0, j1): |dot| > hi is in, |dot| < lo is out, in between the exact distance
void launch_prm_so3_pairs(const PrmArgs& a, uint32_t j0, uint32_t j1, double lo, double hi, double r, hipStream_t s);
void launch_prm_so3_edges(const DevParams& p, const PrmArgs& a, uint32_t n_cand, hipStream_t s);

// prm_revalidate.hip: a roadmap planted from the host, and a roadmap re-checked against the current obstacles
enum PrmPlantRule : uint32_t {   // one result word per rule: the lowest offending row, 0xFFFFFFFF = none; reported in this order
    kPlantOffsetsStart = 0, kPlantOffsetsOrder, kPlantRange, kPlantSelfLoop, kPlantUnsorted, kPlantAsymmetric, kPlantRules
};
enum PrmRevalCounter : uint32_t { kRevalInvalid = 0, kRevalPairs, kRevalCounters };
void launch_prm_shadow(const double* ms, float* ms32, uint64_t count, hipStream_t s);   // (prm_kernels.hip) ms32[i] = fl32(ms[i]), i < count
// off32 = the caller's 64-bit offsets; the rules kPlantOffsetsStart / kPlantOffsetsOrder
void launch_prm_plant_offsets(const uint64_t* off64, uint32_t n, uint32_t* off32, uint32_t* viol, hipStream_t s);
// the per-entry rules; only for offsets that passed the two above
void launch_prm_plant_entries(const uint32_t* offsets, const uint32_t* nbrs, uint32_t n, uint32_t n_entries, uint32_t* viol, hipStream_t s);
void launch_prm_reval_valid(bool so3, const DevParams& p, const double* ms, uint32_t n, uint8_t* valid, uint32_t* counters, hipStream_t s);
// the entries u -> v with v < u and both ends valid, counters[kRevalPairs] of them: pairs[] = (entry, u, v), or -- cand != nullptr --
// cand[] = (u, v) in construction's candidate layout instead
void launch_prm_reval_emit(const uint32_t* offsets, const uint32_t* nbrs, const uint8_t* valid, uint32_t n, uint32_t n_entries, uint4* pairs,
                           uint2* cand, uint32_t pair_cap, uint32_t* counters, hipStream_t s);
// R^n: keep[entry] = keep[mirror entry] = 1 for every pair whose motion u -> v is valid (keep starts at 0)
void launch_prm_reval_check(const DevParams& p, const double* ms, const uint32_t* offsets, const uint32_t* nbrs, uint32_t n, uint32_t n_entries,
                            const uint4* pairs, uint32_t n_pairs, uint8_t* keep, hipStream_t s);
// SO(3): keep[entry of v in row u] = 1 for every directed key (u << shift) | v that launch_prm_so3_edges emitted; state->n_keys of
// them, at most key_cap (one thread each)
void launch_prm_reval_keys(const uint64_t* keys, const PrmState* state, uint32_t key_cap, uint32_t shift, const uint32_t* offsets,
                           const uint32_t* nbrs, uint32_t n, uint8_t* keep, hipStream_t s);
// pos = exclusive scan of keep (rocPRIM); tmp == nullptr queries tmp_bytes
hipError_t prm_reval_scan(void* tmp, size_t& tmp_bytes, const uint8_t* keep, uint32_t* pos, uint32_t n_entries, hipStream_t s);
// offsets in place, the kept neighbours into nbrs_out in their old order (n_entries > 0)
void launch_prm_reval_compact(uint32_t* offsets, const uint32_t* nbrs, const uint8_t* keep, const uint32_t* pos, uint32_t n, uint32_t n_entries,
                              uint32_t* nbrs_out, hipStream_t s);

// prm_grow.hip: what growing a roadmap in place adds to construction's kernels
// keys[e] = (row of CSR entry e << shift) | nbrs[e], e < n_entries
void launch_prm_grow_keys(const uint32_t* offsets, const uint32_t* nbrs, uint32_t n, uint32_t n_entries, uint32_t shift, uint64_t* keys,
                          hipStream_t s);
// the candidates (j, i) whose i is a milestone of this call (i >= n_old) or valid[i] != 0, into out ([n_cand]); *count (zeroed by
// the caller) counts them
void launch_prm_grow_filter(const uint2* cand, uint32_t n_cand, const uint8_t* valid, uint32_t n_old, uint2* out, uint32_t* count,
                            hipStream_t s);

// prm_components.hip: a roadmap's connected components, and the roadmap pruned by a keep mask
enum PrmCcSummary : uint32_t { kCcBest = 0, kCcRoots, kCcSummaryWords };   // (largest size << 32) | (0xFFFFFFFF - its label); the roots
constexpr uint32_t kCcLaunches = 6;   // kernels of one launch_prm_components, whatever the graph
struct PrmCcBuffers {
    uint32_t* parent;              // [n] the union-find forest; scratch once the labels exist
    uint32_t* label;               // [n] the lowest milestone index of the component
    uint32_t* count;               // [n] count[root] = milestones of its component (live ones under `alive`)
    uint32_t* size;                // [n] size[i] = count[label[i]] (0 for a dead i under `alive`)
    unsigned long long* summary;   // [kCcSummaryWords]
};
// the components of the CSR; alive (optional, [n]): a milestone with alive[i] == 0 is a component of its own and its entries
// connect nothing.  Records after_hook / after_flatten (optional) between its phases; returns the kernels launched (kCcLaunches).
uint32_t launch_prm_components(const uint32_t* offsets, const uint32_t* nbrs, const uint8_t* alive, uint32_t n, uint32_t n_entries,
                               const PrmCcBuffers& b, hipEvent_t after_hook, hipEvent_t after_flatten, hipStream_t s);
// keep[i] = (valid == nullptr || valid[i]) && (mask == nullptr || mask[i]); *kept (zeroed by the caller) counts the ones
void launch_prm_prune_stage1(const uint8_t* valid, const uint8_t* mask, uint32_t n, uint8_t* keep, uint32_t* kept, hipStream_t s);
// keep[i] &&= count[label[i]] >= min_size && (!largest || label[i] == the summary's largest label); *kept as above
void launch_prm_prune_stage2(const PrmCcBuffers& b, uint32_t n, uint32_t min_size, bool largest, uint8_t* keep, uint32_t* kept, hipStream_t s);
// new_index[i] = keep[i] ? pos[i] : -1 (pos = exclusive scan of keep); ekeep[e] = both ends of entry e are kept
void launch_prm_prune_flags(const uint32_t* offsets, const uint32_t* nbrs, const uint8_t* keep, const uint32_t* pos, uint32_t n,
                            uint32_t n_entries, int32_t* new_index, uint8_t* ekeep, hipStream_t s);
// the kept entries renumbered into nbrs_out at epos (= exclusive scan of ekeep), the n_kept + 1 new offsets into offsets_out
void launch_prm_prune_entries(const uint32_t* offsets, const uint32_t* nbrs, const uint8_t* ekeep, const uint32_t* epos, const int32_t* new_index,
                              uint32_t n, uint32_t n_entries, uint32_t n_kept, uint32_t* offsets_out, uint32_t* nbrs_out, hipStream_t s);
// row i of ms (AoS [n][dim]) and of ms32 (nullptr: no shadow) to row new_index[i] of ms_out / ms32_out, bit for bit
void launch_prm_prune_states(const double* ms, const float* ms32, const int32_t* new_index, uint32_t n, uint32_t dim, double* ms_out,
                             float* ms32_out, hipStream_t s);

// rrt_revalidate.hip: the trees of an RRT batch re-checked against the current obstacles and compacted in place (DESIGN.md
// section 21).  The per-slot arrays are [P][cap], indexed like DevParams::parent.
struct ProblemState;
struct RevalArgs {
    double* tree;                // DevParams::tree, parent, skip, state, goal_c, goal_thr
    int32_t* parent;
    uint8_t* skip;
    ProblemState* state;
    const double* goal_c;
    const double* goal_thr;
    uint8_t* edge_ok;            // verdict of check_motion(parent[i] -> i); 1 for the root
    uint8_t* alive;              // no edge on the chain to the root failed
    int32_t* new_index;          // survivors below i, -1 for a removed node
    int32_t* jump;               // the survival pass's pointers
    uint32_t* n_after;           // [P] survivors
    uint32_t* n_removed;         // [P]
    uint8_t* goal_lost;          // [P]
    uint32_t cap, tiles;         // tiles: 256-node tiles that cover the largest tree (the grids of the per-node kernels)
    // SO(3): the edges go through launch_so3_check_motion, stage_cap at a time: rows (from, to) AoS [stage_cap][4] and its verdicts
    double* stage_from;
    double* stage_to;
    uint8_t* stage_out;
    uint32_t stage_cap, pad;
    double filt_base;            // the midpoint filter's absolute margin from the bounds and the sphere centres (R^n)
};
void launch_rrt_reval_edges(const DevParams& p, const RevalArgs& a, uint32_t n_problems, hipStream_t s);
void launch_rrt_reval_survive(const RevalArgs& a, uint32_t n_problems, hipStream_t s);
void launch_rrt_reval_scan(const RevalArgs& a, uint32_t n_problems, hipStream_t s);
void launch_rrt_reval_compact(const DevParams& p, const RevalArgs& a, uint32_t n_problems, hipStream_t s);   // + the skip flags

// prm_batch.hip: a batch of queries on the constructed roadmap, breadth-first search and path extraction on the device
// (DESIGN.md section 17).  One round answers the queries [q0, q0 + n_chunk) of the batch; row c of a per-round array is query q0 + c.
struct PrmBatchArgs {
    const double* ms;            // milestones, AoS [n][dim]
    const uint32_t* offsets;     // CSR of the roadmap: node u's neighbours are nbrs[offsets[u] .. offsets[u + 1]), ascending
    const uint32_t* nbrs;
    const double* starts;        // [n_queries][dim]   (whole batch)
    const double* goals;         // [n_queries][dim]
    const double* goal_thr;      // [n_queries] satisfied iff d2 <= goal_thr (SO(3): distance <= goal_thr)
    const double* filt;          // [n_queries] the midpoint filter's absolute margin with this query's start in play (R^n)
    uint8_t* flags;              // [n_chunk][stride] bit 0: start connection, bit 1: goal milestone
    uint32_t* start_valid;       // [n_chunk]
    uint32_t* parent;            // [n_chunk][stride] 0xFFFFFFFF before the search; claim while a level is expanded; then the parent
    uint32_t* queue;             // [n_chunk][stride] the levels back to back: the order in which the reference's FIFO dequeues
    int32_t* status;             // [n_chunk] results of the round
    uint32_t* path_len;
    int32_t* goal_node;
    uint32_t* n_start;
    uint32_t* n_goal;
    uint32_t n, stride, dim, q0, n_chunk, pad;
};
void launch_prm_batch_flags(bool so3, const DevParams& p, const PrmBatchArgs& b, double near, hipStream_t s);   // near: as launch_prm_query's
uint32_t prm_batch_group(uint32_t n, uint64_t n_edge_entries);   // lanes per level node, from the roadmap's mean degree
void launch_prm_batch_search(const PrmBatchArgs& b, uint32_t group, hipStream_t s);
// row_off[c]: first row of query c's path within nodes / rows (this round's rows)
void launch_prm_batch_paths(const PrmBatchArgs& b, const uint64_t* row_off, uint32_t* nodes, double* rows, hipStream_t s);

// prm_shortest.hip: the same batch answered with shortest paths.  The query sets come from the flag
// launchers above and the rows from launch_prm_batch_paths; a round's rows of `label` and `stamp` lie beside those of PrmBatchArgs.
struct PrmShortestArgs {
    const double* w;             // [n_edge_entries] w[e] = distance(ms[u], ms[nbrs[e]]); read in mode 0 only
    uint64_t* label;             // [n_chunk][stride] bit pattern of the label c (a non-negative binary64, +inf = none)
    uint32_t* stamp;             // [n_chunk][stride] the label round that last put the node on a worklist; then its hops
    double* cost;                // [n_chunk] c[goal], +inf unless OXHIP_OK
    uint32_t* rounds;            // [n_chunk] label rounds run
    unsigned long long* relaxed; // [n_chunk] edge relaxations evaluated
    uint32_t mode, pad;          // 0: distance weights, 1: every weight 1.0, 2: every weight 0.0
};
void launch_prm_shortest_weights(bool so3, uint32_t dim, const double* ms, const uint32_t* offsets, const uint32_t* nbrs, uint32_t n,
                                 uint32_t n_entries, double* w, hipStream_t s);
void launch_prm_shortest_init(bool so3, const PrmBatchArgs& b, const PrmShortestArgs& a, hipStream_t s);
void launch_prm_shortest_labels(const PrmBatchArgs& b, const PrmShortestArgs& a, uint32_t group, hipStream_t s);
void launch_prm_shortest_levels(const PrmBatchArgs& b, const PrmShortestArgs& a, uint32_t group, hipStream_t s);

// shortcut_core.hip: the pair matrix and the shortest chain over it, for a round of n_chunk paths (DESIGN.md sections 18 and 25).
// Every pointer is already at the round's first path: path c of the round has len[c] original states, every edge in m parts, and
// its rows, costs, parents and indices begin at row_off[c] of `rows` / cost / par / idx (ShortcutShape, oxhip_host.hpp).
struct ShortcutArgs {
    const uint32_t* len;         // [n_chunk] original states of the path, 0 = none
    const uint64_t* row_off;     // [n_chunk] first row of the path
    const double* rows;          // the paths' rows, (L - 1) m + 1 per path
    const uint64_t* woff;        // [n_chunk + 1] first word of every path's bit matrix within `bits`
    uint64_t* bits;              // bit (d - 2) * M + u of a path: check_motion(q_u, q_{u + d}), 2 <= d <= W, not on one edge
    uint64_t n_words;
    uint32_t n_chunk, m, max_span, pad;
    double filt_base;            // the midpoint filter's absolute margin from the bounds and the sphere centres (R^n)
};
struct ShortcutOut {
    double* cost;                // per row: cost of the best chain from q_0
    uint32_t* par;               // per row: the row before it on that chain
    uint32_t* idx;               // the chain's rows in path order, at the path's first row
    uint32_t* simp_len;          // [n_chunk]
    double* raw_cost;            // [n_chunk]
    double* simp_cost;           // [n_chunk]
    uint64_t* checks;            // [n_chunk] motion checks evaluated
};
// subdivided = false: m is 1 and the space may be SO(2) (an RRT batch); true: R^1 .. R^8 and SO(3) with any m (a PRM batch)
void launch_shortcut_pairs(const DevParams& p, const ShortcutArgs& a, bool subdivided, hipStream_t s);
void launch_shortcut_dp(uint32_t space, uint32_t dim, const ShortcutArgs& a, const ShortcutOut& o, hipStream_t s);

// path_simplify.hip: the solution paths of an RRT / RRTConnect / RRT* batch, extracted on the device.  Problem p's raw path is rows off[p] .. off[p] + len[p] of `rows`.
struct PathArgs {
    const uint64_t* off;         // [P + 1] first row of every problem's path (read by the rows kernel only)
    uint32_t* len;               // [P] states of the path, 0 = unsolved (0xFFFFFFFF from the length kernel: corrupt chain)
    uint32_t* len_a;             // [P] of which from the start tree
    double* rows;                // [total][dim]
};
void launch_path_len(const DevParams& p, const PathArgs& a, hipStream_t s);
void launch_path_rows(const DevParams& p, const PathArgs& a, hipStream_t s);

// prm_path_simplify.hip: the answered paths of a PRM batch, subdivided into m parts per edge for shortcut_core.hip and the chains
// compacted after it.  One round serves the queries [q0, q0 + n_chunk); the dense arrays hold the round's
// dense paths back to back (doff).
struct DenseArgs {
    const uint64_t* off;         // [Q + 1] first raw row of every query's path   (whole batch)
    const double* rows;          // [total][width] the raw rows
    const uint64_t* doff;        // [n_chunk + 1] first dense row of every query of the round
    double* dense;               // [n_rows][width] the dense paths
    uint64_t n_rows;
    uint32_t q0, n_chunk, m, pad;
};
struct DenseOut {
    const uint32_t* simp_len;    // [n_chunk] the chains' lengths ...
    const uint32_t* idx;         // [n_rows] ... and their dense indices in path order, at the query's dense offset
    const uint64_t* soff;        // [n_chunk + 1] first compact row of every query
    uint32_t* out_idx;           // [compact rows]
    double* out_rows;            // [compact rows][width]
};
void launch_dense_rows(bool so3, uint32_t dim, const DenseArgs& a, hipStream_t s);
void launch_dense_gather(uint32_t width, const DenseArgs& a, const DenseOut& g, hipStream_t s);

}  // namespace oxhip
