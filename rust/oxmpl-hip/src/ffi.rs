//! `extern "C"` surface of `liboxmpl_hip.so`, one to one with `include/oxmpl_hip.h`.
//!
//! The layout tables below are data for two checks: `cargo test` compares them with this file's `#[repr(C)]`
//! structs (`offset_of!`), and the repository's CPU test `tests/test_rust_ffi_layout.py` compares them with
//! `offsetof` / `sizeof` as printed by a C program that includes the header, and with the ctypes structures
//! of `oxmpl_amd/capi.py`.  A field added to the header without touching this file fails that test.
#![allow(non_camel_case_types)]

use std::os::raw::c_char;

pub const OXHIP_ABI_VERSION: i32 = 2;
pub const OXHIP_MAX_DIM: usize = 8;

// oxhip_status (mirrors PlanningError, oxmpl/src/base/error.rs:97-108, plus the conditions the reference panics on)
pub const OXHIP_OK: i32 = 0;
pub const OXHIP_ERR_TIMEOUT: i32 = 1;
pub const OXHIP_ERR_NO_SOLUTION_FOUND: i32 = 2;
pub const OXHIP_ERR_PLANNER_UNINITIALISED: i32 = 3;
pub const OXHIP_ERR_INVALID_START_STATE: i32 = 4;
pub const OXHIP_ERR_UNSAMPLED_STATE_SPACE: i32 = 5;
pub const OXHIP_ERR_BAD_ARG: i32 = 16;
pub const OXHIP_ERR_UNBOUNDED: i32 = 17;
pub const OXHIP_ERR_ZERO_VOLUME: i32 = 18;
pub const OXHIP_ERR_CAPACITY: i32 = 19;
pub const OXHIP_ERR_HIP: i32 = 32;
pub const OXHIP_ERR_NO_DEVICE: i32 = 33;

// oxhip_planner_kind / oxhip_kernel_kind / oxhip_space_kind
pub const OXHIP_PLANNER_RRT: u32 = 0;
pub const OXHIP_PLANNER_RRT_CONNECT: u32 = 1;
pub const OXHIP_PLANNER_RRT_STAR: u32 = 2;
pub const OXHIP_KERNEL_AUTO: u32 = 0;
pub const OXHIP_SPACE_REAL_VECTOR: u32 = 0;
pub const OXHIP_SPACE_SE2: u32 = 1;
/// SO3StateSpace (rrt_so3.hip): dim 4, quaternions (x, y, z, w); bounds[0..4] = centre quaternion, bounds[4] = max_angle
pub const OXHIP_SPACE_SO3: u32 = 2;
pub const OXHIP_SPACE_SE3: u32 = 3;
/// SO2StateSpace (rrt_so2.hip): dim 1, bounds[0..1] = (lo, hi), forbidden arcs through `oxhip_rrt_batch_set_boxes`.  The
/// values 4 .. 15 are no space kinds.
pub const OXHIP_SPACE_SO2: u32 = 16;
// oxhip_goal_sampler: what GoalSampleableRegion::sample_goal draws (goal.rs:35-41)
pub const OXHIP_GOAL_SAMPLE_CENTRE: u32 = 0;
pub const OXHIP_GOAL_SAMPLE_UNIFORM_DISC: u32 = 1;

/// `oxhip_rrt_config` (include/oxmpl_hip.h): RRT::new (rrt.rs:75-83) + RealVectorStateSpace::new (rvss.rs:65-100)
/// + the deterministic termination the reference lacks (rrt.rs:226).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct OxhipRrtConfig {
    pub struct_size: u32,
    pub dim: u32,
    pub bounds: [f64; 2 * OXHIP_MAX_DIM],
    pub max_distance: f64,
    pub goal_bias: f64,
    pub lvs_fraction: f64,
    pub n_problems: u32,
    pub max_nodes: u32,
    pub stop_at_goal: u32,
    pub kernel: u32,
    pub seed: u64,
    pub first_problem_id: u64,
    pub device: i32,
    pub planner: u32,
    pub search_radius: f64,
    pub space: u32,
    pub goal_sampler: u32,
    pub debug_flags: u32,
    pub star_pool_share: u32,
    pub frozen_split: u32,
    pub reserved: u32,
}

/// (field, byte offset, byte size) of `oxhip_rrt_config`
pub const OXHIP_RRT_CONFIG_LAYOUT: &[(&str, usize, usize)] = &[
    ("struct_size", 0, 4),
    ("dim", 4, 4),
    ("bounds", 8, 128),
    ("max_distance", 136, 8),
    ("goal_bias", 144, 8),
    ("lvs_fraction", 152, 8),
    ("n_problems", 160, 4),
    ("max_nodes", 164, 4),
    ("stop_at_goal", 168, 4),
    ("kernel", 172, 4),
    ("seed", 176, 8),
    ("first_problem_id", 184, 8),
    ("device", 192, 4),
    ("planner", 196, 4),
    ("search_radius", 200, 8),
    ("space", 208, 4),
    ("goal_sampler", 212, 4),
    ("debug_flags", 216, 4),
    ("star_pool_share", 220, 4),
    ("frozen_split", 224, 4),
    ("reserved", 228, 4),
];
pub const OXHIP_RRT_CONFIG_SIZE: usize = 232;

/// `oxhip_prm_config` (include/oxmpl_hip.h): PRM::new(timeout, connection_radius) (prm.rs:70-78) + the space.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct OxhipPrmConfig {
    pub struct_size: u32,
    pub dim: u32,
    pub bounds: [f64; 2 * OXHIP_MAX_DIM],
    pub timeout: f64,
    pub connection_radius: f64,
    pub lvs_fraction: f64,
    pub max_milestones: u32,
    pub device: i32,
    pub max_samples: u64,
    pub seed: u64,
    pub stream: u64,
    pub knn_k: u32,
    /// `oxhip_space_kind`: OXHIP_SPACE_REAL_VECTOR or OXHIP_SPACE_SO3 (anything else is OXHIP_ERR_BAD_ARG)
    pub space: u32,
}

/// (field, byte offset, byte size) of `oxhip_prm_config`
pub const OXHIP_PRM_CONFIG_LAYOUT: &[(&str, usize, usize)] = &[
    ("struct_size", 0, 4),
    ("dim", 4, 4),
    ("bounds", 8, 128),
    ("timeout", 136, 8),
    ("connection_radius", 144, 8),
    ("lvs_fraction", 152, 8),
    ("max_milestones", 160, 4),
    ("device", 164, 4),
    ("max_samples", 168, 8),
    ("seed", 176, 8),
    ("stream", 184, 8),
    ("knn_k", 192, 4),
    ("space", 196, 4),
];
pub const OXHIP_PRM_CONFIG_SIZE: usize = 200;

/// `oxhip_prm_grow_config` (include/oxmpl_hip.h): what one `oxhip_prm_grow_roadmap` call adds and where its sampler starts.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct OxhipPrmGrowConfig {
    pub struct_size: u32,
    /// milestones to add; 0 is OXHIP_ERR_BAD_ARG
    pub n_more: u32,
    /// sample_uniform calls this call may make; 0 = 4096 * n_more + 2^22
    pub max_samples: u64,
    /// OXHIP_PRM_GROW_NEW_STREAM or 0
    pub flags: u32,
    pub pad: u32,
    /// with OXHIP_PRM_GROW_NEW_STREAM: the ChaCha12 stream id to start at word 0
    pub stream: u64,
}
pub const OXHIP_PRM_GROW_NEW_STREAM: u32 = 1;

/// (field, byte offset, byte size) of `oxhip_prm_grow_config`
pub const OXHIP_PRM_GROW_CONFIG_LAYOUT: &[(&str, usize, usize)] = &[
    ("struct_size", 0, 4),
    ("n_more", 4, 4),
    ("max_samples", 8, 8),
    ("flags", 16, 4),
    ("pad", 20, 4),
    ("stream", 24, 8),
];
pub const OXHIP_PRM_GROW_CONFIG_SIZE: usize = 32;

/// `oxhip_prm_prune_config` (include/oxmpl_hip.h): which milestones one `oxhip_prm_prune` call drops.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct OxhipPrmPruneConfig {
    pub struct_size: u32,
    /// OXHIP_PRM_PRUNE_*, at least one
    pub flags: u32,
    /// with OXHIP_PRM_PRUNE_MIN_SIZE: at least 1
    pub min_size: u32,
    pub pad: u32,
}
pub const OXHIP_PRM_PRUNE_INVALID: u32 = 1;
pub const OXHIP_PRM_PRUNE_MASK: u32 = 2;
pub const OXHIP_PRM_PRUNE_MIN_SIZE: u32 = 4;
pub const OXHIP_PRM_PRUNE_LARGEST: u32 = 8;

/// (field, byte offset, byte size) of `oxhip_prm_prune_config`
pub const OXHIP_PRM_PRUNE_CONFIG_LAYOUT: &[(&str, usize, usize)] = &[
    ("struct_size", 0, 4),
    ("flags", 4, 4),
    ("min_size", 8, 4),
    ("pad", 12, 4),
];
pub const OXHIP_PRM_PRUNE_CONFIG_SIZE: usize = 16;

/// opaque handles (owned by the library; freed with the matching `_destroy`)
#[repr(C)]
pub struct OxhipRrtBatch {
    _private: [u8; 0],
}
#[repr(C)]
pub struct OxhipPrm {
    _private: [u8; 0],
}

extern "C" {
    // ---- library
    pub fn oxhip_abi_version() -> i32;
    pub fn oxhip_status_string(status: i32) -> *const c_char;
    pub fn oxhip_last_error_string() -> *const c_char;
    pub fn oxhip_device_count(count: *mut i32) -> i32;

    // ---- batched tree planners: RRT::new / Planner::setup / Planner::solve (rrt.rs, rrt_connect.rs, rrt_star.rs)
    pub fn oxhip_rrt_batch_create(cfg: *const OxhipRrtConfig, out: *mut *mut OxhipRrtBatch) -> i32;
    pub fn oxhip_rrt_batch_destroy(b: *mut OxhipRrtBatch) -> i32;
    pub fn oxhip_rrt_batch_set_spheres(b: *mut OxhipRrtBatch, centres: *const f64, radii: *const f64, n: u32) -> i32;
    pub fn oxhip_rrt_batch_set_boxes(b: *mut OxhipRrtBatch, lo: *const f64, hi: *const f64, n: u32) -> i32;
    pub fn oxhip_rrt_batch_set_segments(b: *mut OxhipRrtBatch, segments: *const f64, n: u32, clearance: f64) -> i32;
    pub fn oxhip_rrt_batch_set_body(b: *mut OxhipRrtBatch, centres: *const f64, radii: *const f64, n: u32) -> i32;
    pub fn oxhip_rrt_batch_setup(b: *mut OxhipRrtBatch, starts: *const f64, goal_centres: *const f64, goal_radii: *const f64) -> i32;
    pub fn oxhip_rrt_batch_set_tree(b: *mut OxhipRrtBatch, problem: u32, states: *const f64, parents: *const i32, n_nodes: u32) -> i32;
    pub fn oxhip_rrt_batch_solve(b: *mut OxhipRrtBatch, max_iterations: u64, timeout_s: f64, freeze: u32, status_out: *mut i32) -> i32;
    pub fn oxhip_rrt_batch_get_counts(
        b: *mut OxhipRrtBatch,
        iterations: *mut u64,
        nodes: *mut u32,
        accepted: *mut u64,
        checksum: *mut u64,
        goal_node: *mut i32,
        stop_reason: *mut i32,
    ) -> i32;
    pub fn oxhip_rrt_batch_get_tree(b: *mut OxhipRrtBatch, problem: u32, states: *mut f64, parents: *mut i32, cap_nodes: u32, n_nodes: *mut u32) -> i32;
    pub fn oxhip_rrt_batch_get_path(b: *mut OxhipRrtBatch, problem: u32, states: *mut f64, cap_states: u32, len: *mut u32) -> i32;
    pub fn oxhip_rrt_batch_get_goal_counts(b: *mut OxhipRrtBatch, nodes: *mut u32, end_node: *mut i32) -> i32;
    pub fn oxhip_rrt_batch_get_goal_tree(b: *mut OxhipRrtBatch, problem: u32, states: *mut f64, parents: *mut i32, cap_nodes: u32, n_nodes: *mut u32) -> i32;
    pub fn oxhip_rrt_batch_get_costs(b: *mut OxhipRrtBatch, problem: u32, costs: *mut f64, cap_nodes: u32, n_nodes: *mut u32) -> i32;
    pub fn oxhip_rrt_batch_last_timing(b: *mut OxhipRrtBatch, kernel_ms: *mut f64, launches: *mut u32, kernel_kind: *mut u32) -> i32;
    // the whole batch's solution paths, extracted and shortcut on the device (path_simplify.hip, shortcut_core.hip)
    pub fn oxhip_rrt_batch_extract_paths(b: *mut OxhipRrtBatch) -> i32;
    pub fn oxhip_rrt_batch_get_paths(b: *mut OxhipRrtBatch, offsets: *mut u64, states: *mut f64, cap_states: u64, total_out: *mut u64) -> i32;
    pub fn oxhip_rrt_batch_simplify_paths(b: *mut OxhipRrtBatch, max_span: u32, chunk_problems: u32) -> i32;
    pub fn oxhip_rrt_batch_get_simplified_paths(b: *mut OxhipRrtBatch, offsets: *mut u64, states: *mut f64, indices: *mut u32, cap_states: u64, total_out: *mut u64) -> i32;
    pub fn oxhip_rrt_batch_get_simplify_results(b: *mut OxhipRrtBatch, raw_cost: *mut f64, simplified_cost: *mut f64, checks: *mut u64) -> i32;
    pub fn oxhip_rrt_batch_path_valid_matrix(b: *mut OxhipRrtBatch, problem: u32, max_span: u32, out: *mut u8, cap_bytes: u64, len_out: *mut u32) -> i32;
    pub fn oxhip_rrt_batch_paths_last_timing(b: *mut OxhipRrtBatch, extract_ms: *mut f64, pairs_ms: *mut f64, dp_ms: *mut f64, rounds: *mut u32) -> i32;
    pub fn oxhip_rrt_batch_is_valid(b: *mut OxhipRrtBatch, states: *const f64, n: u32, out: *mut u8) -> i32;
    pub fn oxhip_rrt_batch_check_motion(b: *mut OxhipRrtBatch, from: *const f64, to: *const f64, n: u32, out: *mut u8) -> i32;

    // ---- stand-alone pieces of the path (rrt.rs:187-196, rvss.rs:137-155, rvss.rs:161-186)
    pub fn oxhip_nn_argmin_batch(
        device: i32,
        dim: u32,
        nodes: *const f64,
        n_nodes: *const u32,
        n_queries: u32,
        queries: *const f64,
        out_index: *mut u32,
        out_min_dist: *mut f64,
    ) -> i32;
    pub fn oxhip_distance_batch(device: i32, dim: u32, a: *const f64, b: *const f64, n: u32, out: *mut f64) -> i32;
    pub fn oxhip_interpolate_batch(device: i32, dim: u32, from: *const f64, to: *const f64, t: *const f64, n: u32, out: *mut f64) -> i32;
    /// SO(3) self-test hook: op 0 distance, op 1 interpolate, op 2 ox_acos (so3_state_space.rs:101-159)
    pub fn oxhip_so3_op_batch(device: i32, op: u32, a: *const f64, b: *const f64, t: *const f64, n: u32, out: *mut f64) -> i32;
    pub fn oxhip_se3_op_batch(device: i32, op: u32, a: *const f64, b: *const f64, t: *const f64, n: u32, out: *mut f64) -> i32;

    // ---- PRM (prm.rs)
    pub fn oxhip_prm_create(cfg: *const OxhipPrmConfig, out: *mut *mut OxhipPrm) -> i32;
    pub fn oxhip_prm_destroy(p: *mut OxhipPrm) -> i32;
    pub fn oxhip_prm_set_spheres(p: *mut OxhipPrm, centres: *const f64, radii: *const f64, n: u32) -> i32;
    pub fn oxhip_prm_set_boxes(p: *mut OxhipPrm, lo: *const f64, hi: *const f64, n: u32) -> i32;
    pub fn oxhip_prm_setup(p: *mut OxhipPrm, start: *const f64, goal_centre: *const f64, goal_radius: f64) -> i32;
    pub fn oxhip_prm_set_problem(p: *mut OxhipPrm, start: *const f64, goal_centre: *const f64, goal_radius: f64) -> i32;
    pub fn oxhip_prm_construct_roadmap(p: *mut OxhipPrm) -> i32;
    pub fn oxhip_prm_get_sizes(p: *mut OxhipPrm, n_milestones: *mut u32, n_edge_entries: *mut u64, n_samples: *mut u64) -> i32;
    pub fn oxhip_prm_get_roadmap(p: *mut OxhipPrm, states: *mut f64, cap_nodes: u32, offsets: *mut u64, neighbours: *mut u32, cap_entries: u64) -> i32;
    pub fn oxhip_prm_solve(p: *mut OxhipPrm, timeout_s: f64, path: *mut f64, cap_states: u32, len: *mut u32) -> i32;
    pub fn oxhip_prm_get_query_sets(
        p: *mut OxhipPrm,
        start_connections: *mut u32,
        cap_start: u32,
        n_start: *mut u32,
        goal_indices: *mut u32,
        cap_goal: u32,
        n_goal: *mut u32,
    ) -> i32;
    pub fn oxhip_prm_last_timing(p: *mut OxhipPrm, phase_ms: *mut f64, n_candidates: *mut u64, redraw_batches: *mut u32) -> i32;
    pub fn oxhip_prm_knn_exact_rows(p: *mut OxhipPrm, rows: *mut u32) -> i32;
    // a batch of queries on the roadmap as it stands: flags, breadth-first search and paths on the device (prm_batch.hip)
    pub fn oxhip_prm_solve_batch(
        p: *mut OxhipPrm,
        n_queries: u32,
        starts: *const f64,
        goal_centres: *const f64,
        goal_radii: *const f64,
        timeout_s: f64,
        chunk_queries: u32,
        status_out: *mut i32,
    ) -> i32;
    pub fn oxhip_prm_batch_get_results(p: *mut OxhipPrm, status: *mut i32, path_len: *mut u32, goal_node: *mut i32, n_start: *mut u32, n_goal: *mut u32) -> i32;
    pub fn oxhip_prm_batch_get_paths(p: *mut OxhipPrm, offsets: *mut u64, nodes: *mut u32, states: *mut f64, cap_rows: u64, total_rows: *mut u64) -> i32;
    pub fn oxhip_prm_batch_get_query_sets(
        p: *mut OxhipPrm,
        query: u32,
        start_connections: *mut u32,
        cap_start: u32,
        n_start: *mut u32,
        goal_indices: *mut u32,
        cap_goal: u32,
        n_goal: *mut u32,
    ) -> i32;
    pub fn oxhip_prm_batch_last_timing(p: *mut OxhipPrm, phase_ms: *mut f64, rounds: *mut u32) -> i32;
    pub fn oxhip_prm_solve_batch_shortest(
        p: *mut OxhipPrm,
        n_queries: u32,
        starts: *const f64,
        goal_centres: *const f64,
        goal_radii: *const f64,
        timeout_s: f64,
        chunk_queries: u32,
        weights: u32,
        status_out: *mut i32,
    ) -> i32;
    pub fn oxhip_prm_batch_get_costs(p: *mut OxhipPrm, cost: *mut f64) -> i32;
    pub fn oxhip_prm_batch_get_labels(p: *mut OxhipPrm, query: u32, cost: *mut f64, hops: *mut u32, parent: *mut u32, cap: u32) -> i32;
    pub fn oxhip_prm_batch_get_search_stats(p: *mut OxhipPrm, label_rounds: *mut u32, relaxations: *mut u64, phase_ms: *mut f64) -> i32;
    pub fn oxhip_prm_set_roadmap(p: *mut OxhipPrm, states: *const f64, n: u32, offsets: *const u64, neighbours: *const u32) -> i32;
    pub fn oxhip_prm_revalidate(p: *mut OxhipPrm, milestone_valid: *mut u8, n_invalid_milestones: *mut u32, n_removed_entries: *mut u64) -> i32;
    pub fn oxhip_prm_revalidate_last_timing(p: *mut OxhipPrm, phase_ms: *mut f64) -> i32;
    // prm_grow.hip: the roadmap grown in place
    pub fn oxhip_prm_grow_roadmap(p: *mut OxhipPrm, g: *const OxhipPrmGrowConfig, n_added: *mut u32, n_samples_drawn: *mut u64) -> i32;
    pub fn oxhip_prm_grow_last_timing(p: *mut OxhipPrm, phase_ms: *mut f64) -> i32;
    // prm_components.hip: the roadmap's connected components, and the roadmap pruned
    pub fn oxhip_prm_components(p: *mut OxhipPrm, label: *mut u32, size: *mut u32, cap: u32, n_components: *mut u32, largest_label: *mut u32, largest_size: *mut u32) -> i32;
    pub fn oxhip_prm_components_last_timing(p: *mut OxhipPrm, phase_ms: *mut f64, launches: *mut u32) -> i32;
    pub fn oxhip_prm_prune(p: *mut OxhipPrm, c: *const OxhipPrmPruneConfig, keep: *const u8, new_index: *mut i32, n_kept: *mut u32, n_removed_entries: *mut u64) -> i32;
    pub fn oxhip_prm_prune_last_timing(p: *mut OxhipPrm, phase_ms: *mut f64) -> i32;
    pub fn oxhip_prm_is_valid(p: *mut OxhipPrm, states: *const f64, n: u32, out: *mut u8) -> i32;
    pub fn oxhip_prm_check_motion(p: *mut OxhipPrm, from: *const f64, to: *const f64, n: u32, out: *mut u8) -> i32;
    pub fn oxhip_prm_batch_simplify_paths(p: *mut OxhipPrm, subdivide: u32, max_span: u32, chunk_queries: u32) -> i32;
    pub fn oxhip_prm_batch_get_simplified_paths(p: *mut OxhipPrm, offsets: *mut u64, states: *mut f64, indices: *mut u32, cap_rows: u64, total_rows: *mut u64) -> i32;
    pub fn oxhip_prm_batch_get_simplify_results(p: *mut OxhipPrm, raw_cost: *mut f64, simplified_cost: *mut f64, checks: *mut u64) -> i32;
    pub fn oxhip_prm_batch_path_valid_matrix(p: *mut OxhipPrm, query: u32, subdivide: u32, max_span: u32, out: *mut u8, cap_bytes: u64, len_out: *mut u32) -> i32;
    pub fn oxhip_prm_batch_simplify_last_timing(p: *mut OxhipPrm, phase_ms: *mut f64, rounds: *mut u32) -> i32;
    // rrt_revalidate.hip: the trees of an RRT batch re-checked against the current obstacles
    pub fn oxhip_rrt_batch_revalidate_trees(b: *mut OxhipRrtBatch, n_removed: *mut u32, goal_lost: *mut u8) -> i32;
    pub fn oxhip_rrt_batch_get_revalidate_map(b: *mut OxhipRrtBatch, problem: u32, new_index: *mut i32, edge_ok: *mut u8, cap: u32, n_before: *mut u32) -> i32;
    pub fn oxhip_rrt_batch_revalidate_last_timing(b: *mut OxhipRrtBatch, phase_ms: *mut f64) -> i32;
}

#[cfg(test)]
mod tests {
    use super::*;
    use std::mem::{offset_of, size_of};

    macro_rules! check_layout {
        ($ty:ty, $table:expr, $size:expr, [$($field:ident),* $(,)?]) => {{
            assert_eq!(size_of::<$ty>(), $size);
            let mut i = 0;
            $(
                let (name, off, _size) = $table[i];
                assert_eq!(name, stringify!($field));
                assert_eq!(offset_of!($ty, $field), off, "offset of {}", name);
                i += 1;
            )*
            assert_eq!(i, $table.len());
        }};
    }

    #[test]
    fn repr_c_structs_match_the_layout_tables() {
        check_layout!(OxhipRrtConfig, OXHIP_RRT_CONFIG_LAYOUT, OXHIP_RRT_CONFIG_SIZE,
            [struct_size, dim, bounds, max_distance, goal_bias, lvs_fraction, n_problems, max_nodes, stop_at_goal, kernel,
             seed, first_problem_id, device, planner, search_radius, space, goal_sampler, debug_flags, star_pool_share, frozen_split, reserved]);
        check_layout!(OxhipPrmConfig, OXHIP_PRM_CONFIG_LAYOUT, OXHIP_PRM_CONFIG_SIZE,
            [struct_size, dim, bounds, timeout, connection_radius, lvs_fraction, max_milestones, device, max_samples, seed, stream, knn_k, space]);
        check_layout!(OxhipPrmGrowConfig, OXHIP_PRM_GROW_CONFIG_LAYOUT, OXHIP_PRM_GROW_CONFIG_SIZE,
            [struct_size, n_more, max_samples, flags, pad, stream]);
        check_layout!(OxhipPrmPruneConfig, OXHIP_PRM_PRUNE_CONFIG_LAYOUT, OXHIP_PRM_PRUNE_CONFIG_SIZE,
            [struct_size, flags, min_size, pad]);
    }
}
