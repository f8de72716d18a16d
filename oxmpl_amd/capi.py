"""ctypes binding of include/oxmpl_hip.h (the C ABI of liboxmpl_hip.so).

Mirrors the header one to one; numpy arrays in, numpy arrays out.  Nothing here computes:
every call goes into the HIP library, and a missing library or GPU raises.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
# OXMPL_HIP_LIB: development override (kernel tuning experiments load alternative builds)
_LIB = os.environ.get("OXMPL_HIP_LIB") or os.path.join(_PKG, "lib", "liboxmpl_hip.so")

MAX_DIM = 8
OK, ERR_TIMEOUT, ERR_NO_SOLUTION_FOUND, ERR_PLANNER_UNINITIALISED = 0, 1, 2, 3
ERR_INVALID_START_STATE, ERR_UNSAMPLED_STATE_SPACE = 4, 5
ERR_BAD_ARG, ERR_UNBOUNDED, ERR_ZERO_VOLUME, ERR_CAPACITY, ERR_HIP, ERR_NO_DEVICE = 16, 17, 18, 19, 32, 33
STOP_NONE, STOP_GOAL, STOP_ITERATIONS, STOP_NODES, STOP_TIMEOUT = -1, 0, 1, 2, 3
KERNEL_AUTO, KERNEL_STREAM, KERNEL_RESIDENT, KERNEL_LANES, KERNEL_CELLS = 0, 1, 2, 5, 6   # (3 and 4 were retired with ABI version 2)
GOAL_SAMPLE_CENTRE, GOAL_SAMPLE_UNIFORM_DISC = 0, 1
# oxhip_debug_flag: test-only switches that force rarely taken code paths (results identical by construction)
DEBUG_PAIR_TO_WHOLE_TREE, DEBUG_AUDIT, DEBUG_ALL_WHOLE_TREE, DEBUG_ONE_LANE_ROUNDS, DEBUG_SHORT_MEMO = 1, 2, 4, 8, 16
DEBUG_STAR_TWO_PASS, DEBUG_STAR_ONE_SEGMENT = 32, 64
DEBUG_SE2_NO_SEGMENT_GRID = 128
DEBUG_SE2_SMALL_LDS = 256
DEBUG_SO3_SERIAL_SAMPLER = 512
DEBUG_SE3_BRANCHY_SWEEP = 1024
DEBUG_CELLS_NO_PACING = 2048
ABI_VERSION = 2
STAMP_WORDS = 64
STAMP_CELLS_BOARD = 3
PLANNER_RRT, PLANNER_RRT_CONNECT, PLANNER_RRT_STAR = 0, 1, 2
SPACE_REAL_VECTOR, SPACE_SE2, SPACE_SO3, SPACE_SE3 = 0, 1, 2, 3
SPACE_SO2 = 16   # (4 .. 15 are no space kinds)
SE3_MAX_BODY = 16

# every symbol include/oxmpl_hip.h declares (tests check the library exports them all)
EXPORTS = [
    "oxhip_abi_version", "oxhip_status_string", "oxhip_last_error_string", "oxhip_device_count",
    "oxhip_rrt_batch_create", "oxhip_rrt_batch_destroy", "oxhip_rrt_batch_set_spheres",
    "oxhip_rrt_batch_set_boxes", "oxhip_rrt_batch_set_segments", "oxhip_rrt_batch_set_body", "oxhip_rrt_batch_setup", "oxhip_rrt_batch_set_tree", "oxhip_rrt_batch_solve",
    "oxhip_rrt_batch_get_counts", "oxhip_rrt_batch_get_tree", "oxhip_rrt_batch_get_path",
    "oxhip_rrt_batch_get_goal_counts", "oxhip_rrt_batch_get_goal_tree", "oxhip_rrt_batch_get_costs",
    "oxhip_rrt_batch_last_timing", "oxhip_rrt_batch_enable_stamps", "oxhip_rrt_batch_get_stamps",
    "oxhip_nn_argmin_batch", "oxhip_distance_batch",
    "oxhip_interpolate_batch", "oxhip_rrt_batch_is_valid", "oxhip_rrt_batch_check_motion",
    "oxhip_f64_op_batch", "oxhip_se2_op_batch", "oxhip_so3_op_batch", "oxhip_se3_op_batch", "oxhip_rng_u64_batch",
    "oxhip_prm_create", "oxhip_prm_destroy", "oxhip_prm_set_spheres", "oxhip_prm_set_boxes", "oxhip_prm_setup",
    "oxhip_prm_set_problem", "oxhip_prm_construct_roadmap", "oxhip_prm_get_sizes", "oxhip_prm_get_roadmap",
    "oxhip_prm_solve", "oxhip_prm_get_query_sets", "oxhip_prm_last_timing", "oxhip_prm_knn_exact_rows",
    "oxhip_prm_solve_batch", "oxhip_prm_batch_get_results", "oxhip_prm_batch_get_paths", "oxhip_prm_batch_get_query_sets",
    "oxhip_prm_batch_last_timing",
    "oxhip_prm_solve_batch_shortest", "oxhip_prm_batch_get_costs", "oxhip_prm_batch_get_labels", "oxhip_prm_batch_get_search_stats",
    "oxhip_prm_set_roadmap", "oxhip_prm_revalidate", "oxhip_prm_revalidate_last_timing",
    "oxhip_prm_grow_roadmap", "oxhip_prm_grow_last_timing",
    "oxhip_prm_components", "oxhip_prm_components_last_timing", "oxhip_prm_prune", "oxhip_prm_prune_last_timing",
    "oxhip_prm_is_valid", "oxhip_prm_check_motion", "oxhip_prm_batch_simplify_paths", "oxhip_prm_batch_get_simplified_paths",
    "oxhip_prm_batch_get_simplify_results", "oxhip_prm_batch_path_valid_matrix", "oxhip_prm_batch_simplify_last_timing",
    "oxhip_rrt_batch_extract_paths", "oxhip_rrt_batch_get_paths", "oxhip_rrt_batch_simplify_paths",
    "oxhip_rrt_batch_get_simplified_paths", "oxhip_rrt_batch_get_simplify_results", "oxhip_rrt_batch_path_valid_matrix",
    "oxhip_rrt_batch_paths_last_timing",
    "oxhip_rrt_batch_revalidate_trees", "oxhip_rrt_batch_get_revalidate_map", "oxhip_rrt_batch_revalidate_last_timing",
    "oxhip_cells_part_begin", "oxhip_cells_part_quota", "oxhip_cells_problem_quota",
]


class Config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("dim", C.c_uint32), ("bounds", C.c_double * (2 * MAX_DIM)),
        ("max_distance", C.c_double), ("goal_bias", C.c_double), ("lvs_fraction", C.c_double),
        ("n_problems", C.c_uint32), ("max_nodes", C.c_uint32), ("stop_at_goal", C.c_uint32),
        ("kernel", C.c_uint32), ("seed", C.c_uint64), ("first_problem_id", C.c_uint64),
        ("device", C.c_int32), ("planner", C.c_uint32), ("search_radius", C.c_double),
        ("space", C.c_uint32), ("goal_sampler", C.c_uint32), ("debug_flags", C.c_uint32), ("star_pool_share", C.c_uint32),
        ("frozen_split", C.c_uint32), ("reserved", C.c_uint32),
    ]


class PrmConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("dim", C.c_uint32), ("bounds", C.c_double * (2 * MAX_DIM)),
        ("timeout", C.c_double), ("connection_radius", C.c_double), ("lvs_fraction", C.c_double),
        ("max_milestones", C.c_uint32), ("device", C.c_int32), ("max_samples", C.c_uint64),
        ("seed", C.c_uint64), ("stream", C.c_uint64), ("knn_k", C.c_uint32), ("space", C.c_uint32),
    ]


PRM_GROW_NEW_STREAM = 1   # OXHIP_PRM_GROW_NEW_STREAM


class PrmGrowConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_more", C.c_uint32), ("max_samples", C.c_uint64),
        ("flags", C.c_uint32), ("pad", C.c_uint32), ("stream", C.c_uint64),
    ]


PRM_PRUNE_INVALID, PRM_PRUNE_MASK, PRM_PRUNE_MIN_SIZE, PRM_PRUNE_LARGEST = 1, 2, 4, 8   # OXHIP_PRM_PRUNE_*


class PrmPruneConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("min_size", C.c_uint32), ("pad", C.c_uint32)]


class OxhipError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = status
        super().__init__("oxhip status %d (%s)%s" % (status, status_string(status), (": " + detail) if detail else ""))


def library_path():
    return _LIB


def build_library(force=False):
    """hipcc cross-compiles for gfx950 without a GPU; the .so stays in-tree (oxmpl_amd/lib)."""
    csrc = os.path.join(_PKG, "csrc")
    cmd = ["make", "-s", "-C", csrc, "-j4"]
    if force:
        cmd.append("-B")
    subprocess.check_call(cmd)
    return _LIB


_lib = None
_dp = C.POINTER(C.c_double)
_u8p = C.POINTER(C.c_uint8)
_u32p = C.POINTER(C.c_uint32)
_i32p = C.POINTER(C.c_int32)
_u64p = C.POINTER(C.c_uint64)


def lib():
    """Load liboxmpl_hip.so; raises if it has not been built (no fallback of any kind)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB):
            raise OSError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(or make -C oxmpl_amd/csrc). There is no CPU fallback." % _LIB)
        L = C.CDLL(_LIB)
        L.oxhip_abi_version.restype = C.c_int32
        L.oxhip_status_string.restype = C.c_char_p
        L.oxhip_status_string.argtypes = [C.c_int32]
        L.oxhip_last_error_string.restype = C.c_char_p
        L.oxhip_device_count.argtypes = [_i32p]
        L.oxhip_rrt_batch_create.argtypes = [C.POINTER(Config), C.POINTER(C.c_void_p)]
        L.oxhip_rrt_batch_destroy.argtypes = [C.c_void_p]
        L.oxhip_rrt_batch_set_spheres.argtypes = [C.c_void_p, _dp, _dp, C.c_uint32]
        L.oxhip_rrt_batch_set_boxes.argtypes = [C.c_void_p, _dp, _dp, C.c_uint32]
        L.oxhip_rrt_batch_set_segments.argtypes = [C.c_void_p, _dp, C.c_uint32, C.c_double]
        L.oxhip_se2_op_batch.argtypes = [C.c_int32, C.c_uint32, _dp, _dp, _dp, C.c_uint32, _dp]
        L.oxhip_so3_op_batch.argtypes = [C.c_int32, C.c_uint32, _dp, _dp, _dp, C.c_uint32, _dp]
        L.oxhip_rrt_batch_set_body.argtypes = [C.c_void_p, _dp, _dp, C.c_uint32]
        L.oxhip_se3_op_batch.argtypes = [C.c_int32, C.c_uint32, _dp, _dp, _dp, C.c_uint32, _dp]
        L.oxhip_rrt_batch_setup.argtypes = [C.c_void_p, _dp, _dp, _dp]
        L.oxhip_rrt_batch_set_tree.argtypes = [C.c_void_p, C.c_uint32, _dp, _i32p, C.c_uint32]
        L.oxhip_rrt_batch_solve.argtypes = [C.c_void_p, C.c_uint64, C.c_double, C.c_uint32, _i32p]
        L.oxhip_rrt_batch_get_counts.argtypes = [C.c_void_p, _u64p, _u32p, _u64p, _u64p, _i32p, _i32p]
        L.oxhip_rrt_batch_get_tree.argtypes = [C.c_void_p, C.c_uint32, _dp, _i32p, C.c_uint32, _u32p]
        L.oxhip_rrt_batch_get_path.argtypes = [C.c_void_p, C.c_uint32, _dp, C.c_uint32, _u32p]
        L.oxhip_rrt_batch_get_goal_counts.argtypes = [C.c_void_p, _u32p, _i32p]
        L.oxhip_rrt_batch_get_goal_tree.argtypes = [C.c_void_p, C.c_uint32, _dp, _i32p, C.c_uint32, _u32p]
        L.oxhip_rrt_batch_get_costs.argtypes = [C.c_void_p, C.c_uint32, _dp, C.c_uint32, _u32p]
        L.oxhip_rrt_batch_last_timing.argtypes = [C.c_void_p, _dp, _u32p, _u32p]
        L.oxhip_rrt_batch_enable_stamps.argtypes = [C.c_void_p, C.c_uint32]
        L.oxhip_rrt_batch_get_stamps.argtypes = [C.c_void_p, _u64p, C.c_uint32]
        L.oxhip_nn_argmin_batch.argtypes = [C.c_int32, C.c_uint32, _dp, _u32p, C.c_uint32, _dp, _u32p, _dp]
        L.oxhip_distance_batch.argtypes = [C.c_int32, C.c_uint32, _dp, _dp, C.c_uint32, _dp]
        L.oxhip_interpolate_batch.argtypes = [C.c_int32, C.c_uint32, _dp, _dp, _dp, C.c_uint32, _dp]
        L.oxhip_rrt_batch_is_valid.argtypes = [C.c_void_p, _dp, C.c_uint32, _u8p]
        L.oxhip_rrt_batch_check_motion.argtypes = [C.c_void_p, _dp, _dp, C.c_uint32, _u8p]
        L.oxhip_f64_op_batch.argtypes = [C.c_int32, C.c_uint32, _dp, _dp, _dp, C.c_uint32, _dp]
        L.oxhip_rng_u64_batch.argtypes = [C.c_int32, C.c_uint64, C.c_uint64, C.c_uint32, _u64p]
        L.oxhip_prm_create.argtypes = [C.POINTER(PrmConfig), C.POINTER(C.c_void_p)]
        L.oxhip_prm_destroy.argtypes = [C.c_void_p]
        L.oxhip_prm_set_spheres.argtypes = [C.c_void_p, _dp, _dp, C.c_uint32]
        L.oxhip_prm_set_boxes.argtypes = [C.c_void_p, _dp, _dp, C.c_uint32]
        L.oxhip_prm_setup.argtypes = [C.c_void_p, _dp, _dp, C.c_double]
        L.oxhip_prm_set_problem.argtypes = [C.c_void_p, _dp, _dp, C.c_double]
        L.oxhip_prm_construct_roadmap.argtypes = [C.c_void_p]
        L.oxhip_prm_get_sizes.argtypes = [C.c_void_p, _u32p, _u64p, _u64p]
        L.oxhip_prm_get_roadmap.argtypes = [C.c_void_p, _dp, C.c_uint32, _u64p, _u32p, C.c_uint64]
        L.oxhip_prm_solve.argtypes = [C.c_void_p, C.c_double, _dp, C.c_uint32, _u32p]
        L.oxhip_prm_get_query_sets.argtypes = [C.c_void_p, _u32p, C.c_uint32, _u32p, _u32p, C.c_uint32, _u32p]
        L.oxhip_prm_last_timing.argtypes = [C.c_void_p, _dp, _u64p, _u32p]
        L.oxhip_prm_knn_exact_rows.argtypes = [C.c_void_p, _u32p]
        L.oxhip_prm_solve_batch.argtypes = [C.c_void_p, C.c_uint32, _dp, _dp, _dp, C.c_double, C.c_uint32, _i32p]
        L.oxhip_prm_batch_get_results.argtypes = [C.c_void_p, _i32p, _u32p, _i32p, _u32p, _u32p]
        L.oxhip_prm_batch_get_paths.argtypes = [C.c_void_p, _u64p, _u32p, _dp, C.c_uint64, _u64p]
        L.oxhip_prm_batch_get_query_sets.argtypes = [C.c_void_p, C.c_uint32, _u32p, C.c_uint32, _u32p, _u32p, C.c_uint32, _u32p]
        L.oxhip_prm_batch_last_timing.argtypes = [C.c_void_p, _dp, _u32p]
        L.oxhip_prm_solve_batch_shortest.argtypes = [C.c_void_p, C.c_uint32, _dp, _dp, _dp, C.c_double, C.c_uint32, C.c_uint32, _i32p]
        L.oxhip_prm_batch_get_costs.argtypes = [C.c_void_p, _dp]
        L.oxhip_prm_batch_get_labels.argtypes = [C.c_void_p, C.c_uint32, _dp, _u32p, _u32p, C.c_uint32]
        L.oxhip_prm_batch_get_search_stats.argtypes = [C.c_void_p, _u32p, _u64p, _dp]
        L.oxhip_prm_set_roadmap.argtypes = [C.c_void_p, _dp, C.c_uint32, _u64p, _u32p]
        L.oxhip_prm_revalidate.argtypes = [C.c_void_p, _u8p, _u32p, _u64p]
        L.oxhip_prm_revalidate_last_timing.argtypes = [C.c_void_p, _dp]
        L.oxhip_prm_grow_roadmap.argtypes = [C.c_void_p, C.POINTER(PrmGrowConfig), _u32p, _u64p]
        L.oxhip_prm_grow_last_timing.argtypes = [C.c_void_p, _dp]
        L.oxhip_prm_components.argtypes = [C.c_void_p, _u32p, _u32p, C.c_uint32, _u32p, _u32p, _u32p]
        L.oxhip_prm_components_last_timing.argtypes = [C.c_void_p, _dp, _u32p]
        L.oxhip_prm_prune.argtypes = [C.c_void_p, C.POINTER(PrmPruneConfig), _u8p, _i32p, _u32p, _u64p]
        L.oxhip_prm_prune_last_timing.argtypes = [C.c_void_p, _dp]
        L.oxhip_prm_is_valid.argtypes = [C.c_void_p, _dp, C.c_uint32, _u8p]
        L.oxhip_prm_check_motion.argtypes = [C.c_void_p, _dp, _dp, C.c_uint32, _u8p]
        L.oxhip_prm_batch_simplify_paths.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
        L.oxhip_prm_batch_get_simplified_paths.argtypes = [C.c_void_p, _u64p, _dp, _u32p, C.c_uint64, _u64p]
        L.oxhip_prm_batch_get_simplify_results.argtypes = [C.c_void_p, _dp, _dp, _u64p]
        L.oxhip_prm_batch_path_valid_matrix.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, _u8p, C.c_uint64, _u32p]
        L.oxhip_prm_batch_simplify_last_timing.argtypes = [C.c_void_p, _dp, _u32p]
        L.oxhip_rrt_batch_extract_paths.argtypes = [C.c_void_p]
        L.oxhip_rrt_batch_get_paths.argtypes = [C.c_void_p, _u64p, _dp, C.c_uint64, _u64p]
        L.oxhip_rrt_batch_simplify_paths.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        L.oxhip_rrt_batch_get_simplified_paths.argtypes = [C.c_void_p, _u64p, _dp, _u32p, C.c_uint64, _u64p]
        L.oxhip_rrt_batch_get_simplify_results.argtypes = [C.c_void_p, _dp, _dp, _u64p]
        L.oxhip_rrt_batch_path_valid_matrix.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, _u8p, C.c_uint64, _u32p]
        L.oxhip_rrt_batch_paths_last_timing.argtypes = [C.c_void_p, _dp, _dp, _dp, _u32p]
        L.oxhip_rrt_batch_revalidate_trees.argtypes = [C.c_void_p, _u32p, _u8p]
        L.oxhip_rrt_batch_get_revalidate_map.argtypes = [C.c_void_p, C.c_uint32, _i32p, _u8p, C.c_uint32, _u32p]
        L.oxhip_rrt_batch_revalidate_last_timing.argtypes = [C.c_void_p, _dp]
        L.oxhip_cells_part_begin.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
        L.oxhip_cells_part_quota.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
        L.oxhip_cells_problem_quota.argtypes = [C.c_uint32, C.c_uint32]
        for name in EXPORTS:
            if name not in ("oxhip_status_string", "oxhip_last_error_string"):
                getattr(L, name).restype = C.c_int32
        L.oxhip_cells_part_begin.restype = C.c_uint32
        L.oxhip_cells_part_quota.restype = C.c_uint64
        L.oxhip_cells_problem_quota.restype = C.c_uint64
        _lib = L
    return _lib


def status_string(status):
    try:
        return lib().oxhip_status_string(status).decode()
    except OSError:
        return "?"


def _check(status):
    if status != OK:
        raise OxhipError(status, lib().oxhip_last_error_string().decode())


def device_count():
    n = C.c_int32()
    _check(lib().oxhip_device_count(C.byref(n)))
    return n.value


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def _p(a, t=_dp):
    return a.ctypes.data_as(t)


_POINTER = {np.float64: _dp, np.uint8: _u8p, np.uint32: _u32p, np.int32: _i32p, np.uint64: _u64p}


def _sized(fn, lead, buffers, count_type=C.c_uint32, capacity=lambda n: n, fill_empty=True):
    """The ABI's size-then-fill protocol: `fn(*lead, <buffers>, capacity, &count)` is called with null buffers and capacity 0,
    which writes the count (OK or ERR_CAPACITY), then with one array per (dtype, row width; 0: no second axis) of `buffers`.
    An array holds at least one element, so that an empty result still hands the library a buffer.  -> the arrays, cut to
    capacity(count) rows.  fill_empty=False leaves the second call out for a count of 0."""
    n = count_type()
    st = fn(*lead, *([None] * len(buffers)), 0, C.byref(n))
    if st not in (OK, ERR_CAPACITY):
        _check(st)
    cap = capacity(n.value)
    out = [np.zeros((max(cap, 1), width) if width else max(cap, 1), dtype=dtype) for dtype, width in buffers]
    if cap or fill_empty:
        _check(fn(*lead, *[_p(a, _POINTER[dtype]) for a, (dtype, _) in zip(out, buffers)], cap, C.byref(n)))
    return [a[:cap] for a in out]


def _phase_ms(fn, h, n_phases, *scalars):
    """a *_last_timing entry point: n_phases HIP-event times in ms, then `scalars` (ctypes objects, written in place)"""
    ms = np.zeros(n_phases, dtype=np.float64)
    _check(fn(h, _p(ms), *[C.byref(x) for x in scalars]))
    return ms


def _fill_bounds(cfg, dim, bounds, space, se3=False):
    """cfg.dim and cfg.bounds of a Config / PrmConfig from a flat or nested `bounds`: how many values the space kind asks for is
    checked here, what they are by the library.  se3: the entry point reads SE(3)'s eleven values (one that does not gets dim
    pairs and refuses the kind itself)."""
    cfg.dim = dim
    b = _f64(bounds).reshape(-1)
    if space == SPACE_SO3:
        if b.size != 5:
            raise OxhipError(ERR_BAD_ARG, "SO(3) bounds are (cx, cy, cz, cw, max_angle)")
    elif se3 and space == SPACE_SE3:
        if b.size != 11:
            raise OxhipError(ERR_BAD_ARG, "SE(3) bounds are (x lo, x hi, y lo, y hi, z lo, z hi, cx, cy, cz, cw, max_angle)")
    elif b.size != 2 * dim:
        raise OxhipError(ERR_BAD_ARG, "bounds must hold dim (lo,hi) pairs")  # StateSpaceError::DimensionMismatch
    for i, v in enumerate(b[:2 * MAX_DIM]):  # dim > MAX_DIM is rejected by the library
        cfg.bounds[i] = v


class _Handle:
    """What RRTBatch and PRMRoadmap share: the life of the library's handle and the sphere / box uploads.  `_ABI` is the
    prefix of the class's entry points."""

    def _fn(self, name):
        return getattr(lib(), self._ABI + name)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._fn("destroy")(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def set_spheres(self, centres, radii):
        r = _f64(radii).reshape(-1)
        c = _f64(centres, (r.size, 3 if self.space == SPACE_SE3 else self.dim))
        _check(self._fn("set_spheres")(self._h, _p(c), _p(r), r.size))

    def set_boxes(self, lo, hi):
        lo = _f64(lo).reshape(-1, self.dim)
        hi = _f64(hi, lo.shape)
        _check(self._fn("set_boxes")(self._h, _p(lo), _p(hi), lo.shape[0]))


class RRTBatch(_Handle):
    """P independent oxmpl RRT planners (RealVectorStateSpace, ball goal, sphere/box validity)
    grown on one GPU.  Thin wrapper of the oxhip_rrt_batch_* entry points.

    space=SPACE_SO3 (dim 4, quaternions (x, y, z, w)): `bounds` is (cx, cy, cz, cw, max_angle) -- SO3StateSpace's centre
    quaternion and cone of freedom, as include/oxmpl_hip.h reinterprets the config's bounds -- and set_spheres takes the
    forbidden cones (centre quaternion, radius in the SO(3) distance).

    space=SPACE_SO2 (dim 1, one angle per state, taken as given): `bounds` is (lo, hi), clamped to [-PI, PI] by the library, and
    set_boxes takes the forbidden arcs as 1-wide rows: lo = the arcs' minima, hi = their maxima.

    space=SPACE_SE3 (dim 7, states (x, y, z, qx, qy, qz, qw); planner=PLANNER_RRT_CONNECT): `bounds` holds eleven values, the
    (lo, hi) pairs of x, y, z and then (cx, cy, cz, cw, max_angle) of the rotation; set_body gives the rigid body's spheres
    and set_spheres the world's (3-wide centres)."""
    _ABI = "oxhip_rrt_batch_"

    def __init__(self, dim, bounds, max_distance, goal_bias, n_problems, max_nodes=10000,
                 lvs_fraction=0.05, stop_at_goal=True, seed=0, first_problem_id=0, device=0,
                 kernel=KERNEL_AUTO, planner=PLANNER_RRT, search_radius=0.0, space=SPACE_REAL_VECTOR,
                 goal_sampler=GOAL_SAMPLE_CENTRE, debug_flags=0, star_pool_share=0, frozen_split=0):
        cfg = Config()
        cfg.struct_size = C.sizeof(Config)
        _fill_bounds(cfg, dim, bounds, space, se3=True)
        cfg.max_distance, cfg.goal_bias, cfg.lvs_fraction = max_distance, goal_bias, lvs_fraction
        cfg.n_problems, cfg.max_nodes = n_problems, max_nodes
        cfg.stop_at_goal, cfg.kernel = int(bool(stop_at_goal)), kernel
        cfg.seed, cfg.first_problem_id, cfg.device = seed, first_problem_id, device
        cfg.planner = planner
        cfg.search_radius = search_radius
        cfg.space = space
        cfg.goal_sampler, cfg.debug_flags, cfg.star_pool_share = goal_sampler, debug_flags, star_pool_share
        cfg.frozen_split = frozen_split
        self.planner, self.space = planner, space
        self.dim, self.n_problems, self.max_nodes = dim, n_problems, max_nodes
        self._h = C.c_void_p()
        _check(lib().oxhip_rrt_batch_create(C.byref(cfg), C.byref(self._h)))

    def set_segments(self, segments, clearance):
        """SE(2) batches: the segment-soup checker (disc robot of radius `clearance`)"""
        s = _f64(segments).reshape(-1, 4)
        _check(lib().oxhip_rrt_batch_set_segments(self._h, _p(s), s.shape[0], clearance))

    def set_body(self, centres, radii):
        """SE(3) batches: the rigid body's spheres (1 .. 16), centres [n][3] in the body frame"""
        r = _f64(radii).reshape(-1)
        c = _f64(centres).reshape(-1, 3)
        if c.shape[0] != r.size:
            raise OxhipError(ERR_BAD_ARG, "one radius per body sphere")
        _check(lib().oxhip_rrt_batch_set_body(self._h, _p(c), _p(r), r.size))

    def setup(self, starts, goal_centres, goal_radii):
        P = self.n_problems
        s = np.ascontiguousarray(np.broadcast_to(_f64(starts).reshape(-1, self.dim), (P, self.dim)))
        g = np.ascontiguousarray(np.broadcast_to(_f64(goal_centres).reshape(-1, self.dim), (P, self.dim)))
        r = np.ascontiguousarray(np.broadcast_to(_f64(goal_radii).reshape(-1), (P,)))
        _check(lib().oxhip_rrt_batch_setup(self._h, _p(s), _p(g), _p(r)))

    def set_tree(self, problem, states, parents):
        s = _f64(states).reshape(-1, self.dim)
        par = np.ascontiguousarray(parents, dtype=np.int32)
        _check(lib().oxhip_rrt_batch_set_tree(self._h, problem, _p(s), _p(par, _i32p), s.shape[0]))

    def solve(self, max_iterations, timeout_s=0.0, freeze=False):
        st = np.empty(self.n_problems, dtype=np.int32)
        _check(lib().oxhip_rrt_batch_solve(self._h, int(max_iterations), float(timeout_s), int(bool(freeze)),
                                           _p(st, _i32p)))
        return st

    def counts(self):
        P = self.n_problems
        out = dict(iterations=np.empty(P, np.uint64), nodes=np.empty(P, np.uint32), accepted=np.empty(P, np.uint64),
                   checksum=np.empty(P, np.uint64), goal_node=np.empty(P, np.int32), stop_reason=np.empty(P, np.int32))
        _check(lib().oxhip_rrt_batch_get_counts(self._h, _p(out["iterations"], _u64p), _p(out["nodes"], _u32p),
                                                _p(out["accepted"], _u64p), _p(out["checksum"], _u64p),
                                                _p(out["goal_node"], _i32p), _p(out["stop_reason"], _i32p)))
        return out

    def tree(self, problem):
        return tuple(_sized(lib().oxhip_rrt_batch_get_tree, (self._h, problem), [(np.float64, self.dim), (np.int32, 0)]))

    def costs(self, problem):
        """RRT*: Node::cost of every node (rrt_star.rs:26)"""
        return _sized(lib().oxhip_rrt_batch_get_costs, (self._h, problem), [(np.float64, 0)])[0]

    def goal_counts(self):
        """RRTConnect: goal-tree sizes and the last goal-tree node of each solution"""
        P = self.n_problems
        nodes, end = np.empty(P, np.uint32), np.empty(P, np.int32)
        _check(lib().oxhip_rrt_batch_get_goal_counts(self._h, _p(nodes, _u32p), _p(end, _i32p)))
        return dict(nodes=nodes, end_node=end)

    def goal_tree(self, problem):
        return tuple(_sized(lib().oxhip_rrt_batch_get_goal_tree, (self._h, problem), [(np.float64, self.dim), (np.int32, 0)]))

    def path(self, problem):
        return _sized(lib().oxhip_rrt_batch_get_path, (self._h, problem), [(np.float64, self.dim)], fill_empty=False)[0]

    # ---- the whole batch's paths: extraction and shortcutting on the device

    def extract_paths(self):
        """Walk every solved problem's parent chain on the device; paths() then hands all of them out in one copy."""
        _check(lib().oxhip_rrt_batch_extract_paths(self._h))

    def paths(self):
        """(offsets [P+1] u64, rows [total][dim]): problem p's path is rows offsets[p] .. offsets[p+1], bit for bit path(p)"""
        offsets = np.zeros(self.n_problems + 1, dtype=np.uint64)
        rows, = _sized(lib().oxhip_rrt_batch_get_paths, (self._h, _p(offsets, _u64p)), [(np.float64, self.dim)], C.c_uint64)
        return offsets, rows

    def simplify_paths(self, max_span=0, chunk_problems=0):
        """Shortcut every path over its own waypoints (include/oxmpl_hip.h states the semantics); extracts the paths first
        if that has not been done.  chunk_problems: problems per device round (test-only; results never depend on it)."""
        _check(lib().oxhip_rrt_batch_simplify_paths(self._h, int(max_span), int(chunk_problems)))

    def simplified_paths(self):
        """(offsets [P+1] u64, rows [total][dim], indices [total] u32 into the raw path, raw_cost [P], simplified_cost [P],
        checks [P] u64)"""
        P = self.n_problems
        offsets = np.zeros(P + 1, dtype=np.uint64)
        rows, idx = _sized(lib().oxhip_rrt_batch_get_simplified_paths, (self._h, _p(offsets, _u64p)),
                           [(np.float64, self.dim), (np.uint32, 0)], C.c_uint64)
        raw, simp, checks = np.zeros(P), np.zeros(P), np.zeros(P, dtype=np.uint64)
        _check(lib().oxhip_rrt_batch_get_simplify_results(self._h, _p(raw), _p(simp), _p(checks, _u64p)))
        return offsets, rows, idx, raw, simp, checks

    def path_valid_matrix(self, problem, max_span=0):
        """test hook: valid(i, j) of the extracted path of `problem` as the pair kernel evaluates it, [L][L] bool (i < j)"""
        out, = _sized(lib().oxhip_rrt_batch_path_valid_matrix, (self._h, problem, int(max_span)), [(np.uint8, 0)],
                      capacity=lambda L: L * L)    # the count is the path's length L, the buffer holds L * L verdicts
        L = math.isqrt(out.size)
        return out.reshape(L, L).astype(bool)

    def paths_last_timing(self):
        """dict(extract_ms, pairs_ms, dp_ms, rounds): HIP-event times of the last extract_paths / simplify_paths"""
        e, pr, dp, r = C.c_double(), C.c_double(), C.c_double(), C.c_uint32()
        _check(lib().oxhip_rrt_batch_paths_last_timing(self._h, C.byref(e), C.byref(pr), C.byref(dp), C.byref(r)))
        return dict(extract_ms=e.value, pairs_ms=pr.value, dp_ms=dp.value, rounds=r.value)

    # ---- the trees re-checked against the obstacles as they are now

    def revalidate_trees(self):
        """Re-check every tree edge against the current spheres / boxes / cones, drop every node whose chain to the root holds a
        failed edge, compact in place (include/oxmpl_hip.h states the semantics) -> dict(n_removed [P] u32, goal_lost [P] bool)"""
        P = self.n_problems
        removed, lost = np.zeros(P, dtype=np.uint32), np.zeros(P, dtype=np.uint8)
        _check(lib().oxhip_rrt_batch_revalidate_trees(self._h, _p(removed, _u32p), _p(lost, _u8p)))
        return dict(n_removed=removed, goal_lost=lost.astype(bool))

    def revalidate_map(self, problem):
        """(new_index [n_before] i32, edge_ok [n_before] bool) of the last revalidate_trees: where every old node went (-1:
        removed) and the verdict of its edge from its parent (the root's is True)"""
        new_index, edge_ok = _sized(lib().oxhip_rrt_batch_get_revalidate_map, (self._h, problem), [(np.int32, 0), (np.uint8, 0)])
        return new_index, edge_ok.astype(bool)

    def revalidate_last_timing(self):
        """dict(phase_ms=[edge checks, survival, scan, compaction + remap + skip flags]) of the last revalidate_trees"""
        return dict(phase_ms=_phase_ms(lib().oxhip_rrt_batch_revalidate_last_timing, self._h, 4))

    def last_timing(self):
        ms, launches, kind = C.c_double(), C.c_uint32(), C.c_uint32()
        _check(lib().oxhip_rrt_batch_last_timing(self._h, C.byref(ms), C.byref(launches), C.byref(kind)))
        return dict(kernel_ms=ms.value, launches=launches.value, kernel=kind.value)

    def enable_stamps(self, enable=True):
        _check(lib().oxhip_rrt_batch_enable_stamps(self._h, int(bool(enable))))

    def stamps(self):
        out = np.zeros(STAMP_WORDS, dtype=np.uint64)
        _check(lib().oxhip_rrt_batch_get_stamps(self._h, _p(out, _u64p), STAMP_WORDS))
        return out

    def is_valid(self, states):
        s = _f64(states).reshape(-1, self.dim)
        out = np.empty(s.shape[0], dtype=np.uint8)
        _check(lib().oxhip_rrt_batch_is_valid(self._h, _p(s), s.shape[0], _p(out, _u8p)))
        return out.astype(bool)

    def check_motion(self, frm, to):
        a = _f64(frm).reshape(-1, self.dim)
        b = _f64(to, a.shape)
        out = np.empty(a.shape[0], dtype=np.uint8)
        _check(lib().oxhip_rrt_batch_check_motion(self._h, _p(a), _p(b), a.shape[0], _p(out, _u8p)))
        return out.astype(bool)


def nn_argmin_batch(trees, queries, device=0):
    """trees: list of [n_i, dim] arrays; queries: [Q, dim] -> (index[Q], min_dist[Q])  (rrt.rs:187-196)"""
    q = _f64(queries)
    dim = q.shape[1]
    n = np.array([t.shape[0] for t in trees], dtype=np.uint32)
    nodes = _f64(np.concatenate([_f64(t).reshape(-1, dim) for t in trees], axis=0))
    idx = np.empty(len(trees), dtype=np.uint32)
    md = np.empty(len(trees), dtype=np.float64)
    _check(lib().oxhip_nn_argmin_batch(device, dim, _p(nodes), _p(n, _u32p), len(trees), _p(q), _p(idx, _u32p), _p(md)))
    return idx, md


def distance_batch(a, b, device=0):
    a = _f64(a)
    b = _f64(b, a.shape)
    out = np.empty(a.shape[0], dtype=np.float64)
    _check(lib().oxhip_distance_batch(device, a.shape[1], _p(a), _p(b), a.shape[0], _p(out)))
    return out


def interpolate_batch(frm, to, t, device=0):
    a = _f64(frm)
    b = _f64(to, a.shape)
    t = _f64(t).reshape(-1)
    out = np.empty_like(a)
    _check(lib().oxhip_interpolate_batch(device, a.shape[1], _p(a), _p(b), _p(t), a.shape[0], _p(out)))
    return out


def f64_op_batch(op, a, b=None, c=None, device=0):
    a = _f64(a).reshape(-1)
    b = None if b is None else _f64(b, a.shape)
    c = None if c is None else _f64(c, a.shape)
    out = np.empty_like(a)
    _check(lib().oxhip_f64_op_batch(device, op, _p(a), None if b is None else _p(b), None if c is None else _p(c),
                                    a.size, _p(out)))
    return out


def rng_u64_batch(seed, stream, n, device=0):
    out = np.empty(n, dtype=np.uint64)
    _check(lib().oxhip_rng_u64_batch(device, seed, stream, n, _p(out, _u64p)))
    return out


def se2_op_batch(op, a, b, t=None, device=0):
    """op 0: rows (se2_distance, so2_normalise(a.theta), so2_distance(a.theta, b.theta)); op 1: se2_interpolate"""
    a, b = _f64(a).reshape(-1, 3), _f64(b).reshape(-1, 3)
    out = np.empty_like(a)
    tt = None if t is None else _f64(t).reshape(-1)
    _check(lib().oxhip_se2_op_batch(device, op, _p(a), _p(b), None if tt is None else _p(tt), a.shape[0], _p(out)))
    return out


def so3_op_batch(op, a, b=None, t=None, device=0):
    """SO(3) arithmetic on the device: op 0 distance(a_i, b_i) -> [n]; op 1 interpolate(a_i, b_i, t_i) -> [n, 4];
    op 2 ox_acos(a_i) of n scalars -> [n]"""
    if op == 2:
        a = _f64(a).reshape(-1)
        out = np.empty(a.size, dtype=np.float64)
        _check(lib().oxhip_so3_op_batch(device, op, _p(a), None, None, a.size, _p(out)))
        return out
    a, b = _f64(a).reshape(-1, 4), _f64(b).reshape(-1, 4)
    out = np.empty((a.shape[0], 4) if op == 1 else a.shape[0], dtype=np.float64)
    tt = None if t is None else _f64(t).reshape(-1)
    _check(lib().oxhip_so3_op_batch(device, op, _p(a), _p(b), None if tt is None else _p(tt), a.shape[0], _p(out)))
    return out


def se3_op_batch(op, a, b, t=None, device=0):
    """rows (x, y, z, qx, qy, qz, qw).  op 0: distance(a, b) [n]; op 1: interpolate(a, b, t) [n][7];
    op 2: rot(q of a, first three of b) + xyz of a [n][3]"""
    a = _f64(a).reshape(-1, 7)
    b = _f64(b, a.shape)
    tt = None if t is None else _f64(t, (a.shape[0],))
    out = np.empty(a.shape[0] if op == 0 else (a.shape[0], 7 if op == 1 else 3), dtype=np.float64)
    _check(lib().oxhip_se3_op_batch(device, op, _p(a), _p(b), None if tt is None else _p(tt), a.shape[0], _p(out)))
    return out


class PRMRoadmap(_Handle):
    """oxmpl's PRM (prm.rs) on one GPU: roadmap construction and queries.  Thin wrapper of oxhip_prm_*.

    space=SPACE_SO3 (dim 4, quaternions (x, y, z, w)): `bounds` is (cx, cy, cz, cw, max_angle), as for RRTBatch, and
    set_spheres takes the forbidden cones (centre quaternion, radius in the SO(3) distance)."""
    _ABI = "oxhip_prm_"

    def __init__(self, dim, bounds, connection_radius, max_milestones, timeout=0.0, lvs_fraction=0.05,
                 max_samples=0, seed=0, stream=0, device=0, knn_k=0, space=SPACE_REAL_VECTOR):
        cfg = PrmConfig()
        cfg.struct_size = C.sizeof(PrmConfig)
        _fill_bounds(cfg, dim, bounds, space)
        cfg.timeout, cfg.connection_radius, cfg.lvs_fraction = timeout, connection_radius, lvs_fraction
        cfg.max_milestones, cfg.device, cfg.max_samples = max_milestones, device, max_samples
        cfg.seed, cfg.stream = seed, stream
        cfg.knn_k = knn_k   # 0: radius connection (the reference); k > 0: connect to the k nearest earlier milestones
        cfg.space = space
        self.dim, self.space = dim, space
        self._h = C.c_void_p()
        _check(lib().oxhip_prm_create(C.byref(cfg), C.byref(self._h)))

    def setup(self, start, goal_centre, goal_radius):
        s, g = _f64(start, (self.dim,)), _f64(goal_centre, (self.dim,))
        _check(lib().oxhip_prm_setup(self._h, _p(s), _p(g), goal_radius))

    def set_problem(self, start, goal_centre, goal_radius):
        s, g = _f64(start, (self.dim,)), _f64(goal_centre, (self.dim,))
        _check(lib().oxhip_prm_set_problem(self._h, _p(s), _p(g), goal_radius))

    def construct_roadmap(self):
        _check(lib().oxhip_prm_construct_roadmap(self._h))

    def sizes(self):
        """(milestones, edge entries = 2 x undirected edges, samples drawn)"""
        n, e, s = C.c_uint32(), C.c_uint64(), C.c_uint64()
        _check(lib().oxhip_prm_get_sizes(self._h, C.byref(n), C.byref(e), C.byref(s)))
        return n.value, e.value, s.value

    def roadmap(self):
        """(states [n][dim], offsets [n+1] u64, neighbours [E] u32)"""
        n, e, _ = self.sizes()
        states = np.zeros((n, self.dim), dtype=np.float64)
        offsets = np.zeros(n + 1, dtype=np.uint64)
        nbrs = np.zeros(max(e, 1), dtype=np.uint32)
        _check(lib().oxhip_prm_get_roadmap(self._h, _p(states), n, _p(offsets, _u64p), _p(nbrs, _u32p), e))
        return states, offsets, nbrs[:e]

    def solve(self, timeout_s=0.0):
        """Planner::solve: returns (status, path [len][dim]); the status codes mirror PlanningError"""
        ln = C.c_uint32()
        st = lib().oxhip_prm_solve(self._h, timeout_s, None, 0, C.byref(ln))
        if st != OK:
            if st in (ERR_TIMEOUT, ERR_NO_SOLUTION_FOUND, ERR_PLANNER_UNINITIALISED, ERR_INVALID_START_STATE,
                      ERR_UNSAMPLED_STATE_SPACE):
                return st, np.zeros((0, self.dim))
            _check(st)
        path = np.zeros((ln.value, self.dim), dtype=np.float64)
        _check(lib().oxhip_prm_solve(self._h, timeout_s, _p(path), ln.value, C.byref(ln)))
        return OK, path

    def query_sets(self):
        ns, ng = C.c_uint32(), C.c_uint32()
        _check(lib().oxhip_prm_get_query_sets(self._h, None, 0, C.byref(ns), None, 0, C.byref(ng)))
        sc = np.zeros(max(ns.value, 1), dtype=np.uint32)
        gi = np.zeros(max(ng.value, 1), dtype=np.uint32)
        _check(lib().oxhip_prm_get_query_sets(self._h, _p(sc, _u32p), ns.value, C.byref(ns), _p(gi, _u32p), ng.value,
                                              C.byref(ng)))
        return sc[:ns.value], gi[:ng.value]

    def knn_exact_rows(self):
        """k-nearest variant: rows of the last construct_roadmap that were searched exactly (their candidate radius fell short)"""
        r = C.c_uint32()
        _check(lib().oxhip_prm_knn_exact_rows(self._h, C.byref(r)))
        return r.value

    def last_timing(self):
        """dict(phase_ms=[sample, pairs, edges, sort+csr, query, bfs], candidates, redraw_batches)"""
        c, r = C.c_uint64(), C.c_uint32()
        ms = _phase_ms(lib().oxhip_prm_last_timing, self._h, 6, c, r)
        return dict(phase_ms=ms.tolist(), candidates=c.value, redraw_batches=r.value)

    # ---- a batch of queries on the roadmap as it stands: flags, breadth-first search and paths on the device

    def solve_batch(self, starts, goal_centres, goal_radii, timeout_s=0.0, chunk_queries=0):
        """Q (start, ball goal) queries in one call, each answered exactly as set_problem + solve answer it.
        Returns the per-query statuses [Q] (OK, ERR_INVALID_START_STATE, ERR_NO_SOLUTION_FOUND, ERR_TIMEOUT)."""
        return self._solve_batch(lib().oxhip_prm_solve_batch, starts, goal_centres, goal_radii, timeout_s, chunk_queries)

    def _solve_batch(self, fn, starts, goal_centres, goal_radii, timeout_s, *options):
        r = _f64(goal_radii).reshape(-1)
        s, g = _f64(starts, (r.size, self.dim)), _f64(goal_centres, (r.size, self.dim))
        status = np.zeros(max(r.size, 1), dtype=np.int32)
        _check(fn(self._h, r.size, _p(s), _p(g), _p(r), timeout_s, *options, _p(status, _i32p)))
        self._batch_q = r.size
        return status[:r.size]

    def batch_results(self):
        """dict(status, path_len, goal_node, n_start, n_goal), one entry per query of the last batch"""
        q = getattr(self, "_batch_q", 0)
        st, gn = np.zeros(max(q, 1), dtype=np.int32), np.zeros(max(q, 1), dtype=np.int32)
        ln, ns, ng = (np.zeros(max(q, 1), dtype=np.uint32) for _ in range(3))
        _check(lib().oxhip_prm_batch_get_results(self._h, _p(st, _i32p), _p(ln, _u32p), _p(gn, _i32p), _p(ns, _u32p), _p(ng, _u32p)))
        return dict(status=st[:q], path_len=ln[:q], goal_node=gn[:q], n_start=ns[:q], n_goal=ng[:q])

    def batch_paths(self):
        """(offsets [Q+1] u64, nodes [rows] u32, states [rows][dim]): query q's path is rows offsets[q] .. offsets[q+1]"""
        q = getattr(self, "_batch_q", 0)
        offsets = np.zeros(q + 1, dtype=np.uint64)
        total = C.c_uint64()
        _check(lib().oxhip_prm_batch_get_paths(self._h, _p(offsets, _u64p), None, None, 0, C.byref(total)))
        nodes = np.zeros(max(total.value, 1), dtype=np.uint32)
        states = np.zeros((max(total.value, 1), self.dim), dtype=np.float64)
        _check(lib().oxhip_prm_batch_get_paths(self._h, _p(offsets, _u64p), _p(nodes, _u32p), _p(states), total.value, C.byref(total)))
        return offsets, nodes[:total.value], states[:total.value]

    def batch_query_sets(self, query):
        """(start_connections, goal_indices) of query `query` of the last batch"""
        ns, ng = C.c_uint32(), C.c_uint32()
        _check(lib().oxhip_prm_batch_get_query_sets(self._h, query, None, 0, C.byref(ns), None, 0, C.byref(ng)))
        sc = np.zeros(max(ns.value, 1), dtype=np.uint32)
        gi = np.zeros(max(ng.value, 1), dtype=np.uint32)
        _check(lib().oxhip_prm_batch_get_query_sets(self._h, query, _p(sc, _u32p), ns.value, C.byref(ns), _p(gi, _u32p), ng.value,
                                                    C.byref(ng)))
        return sc[:ns.value], gi[:ng.value]

    def batch_last_timing(self):
        """dict(phase_ms=[flags, search, paths, copies], rounds) of the last batch"""
        r = C.c_uint32()
        ms = _phase_ms(lib().oxhip_prm_batch_last_timing, self._h, 4, r)
        return dict(phase_ms=ms.tolist(), rounds=r.value)

    # ---- the same batch answered with shortest paths

    def solve_batch_shortest(self, starts, goal_centres, goal_radii, timeout_s=0.0, chunk_queries=0, weights=0):
        """Q queries in one call, each answered with a shortest path on the roadmap: weights 0 = the space's distance, 1 = unit
        (fewest hops), 2 = zero (test only).  Statuses and query sets are solve_batch's; batch_results / batch_paths /
        batch_query_sets / batch_last_timing serve this batch as they serve solve_batch's."""
        return self._solve_batch(lib().oxhip_prm_solve_batch_shortest, starts, goal_centres, goal_radii, timeout_s, chunk_queries,
                                 weights)

    def batch_costs(self):
        """the label of the goal milestone reached, per query of the last shortest-path batch (+inf unless OK)"""
        q = getattr(self, "_batch_q", 0)
        cost = np.zeros(max(q, 1), dtype=np.float64)
        _check(lib().oxhip_prm_batch_get_costs(self._h, _p(cost)))
        return cost[:q]

    def batch_labels(self, query):
        """(cost [n], hops [n], parent [n]) of every milestone for query `query` of the last shortest-path batch"""
        n = self.sizes()[0]
        cost = np.zeros(max(n, 1), dtype=np.float64)
        hops, parent = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
        _check(lib().oxhip_prm_batch_get_labels(self._h, query, _p(cost), _p(hops, _u32p), _p(parent, _u32p), n))
        return cost[:n], hops[:n], parent[:n]

    def batch_search_stats(self):
        """dict(label_rounds [Q], relaxations [Q], phase_ms=[weights, flags, labels, levels, paths, copies]) of the last shortest-path batch"""
        q = getattr(self, "_batch_q", 0)
        rounds, relax, ms = np.zeros(max(q, 1), dtype=np.uint32), np.zeros(max(q, 1), dtype=np.uint64), np.zeros(6, dtype=np.float64)
        _check(lib().oxhip_prm_batch_get_search_stats(self._h, _p(rounds, _u32p), _p(relax, _u64p), _p(ms)))
        return dict(label_rounds=rounds[:q], relaxations=relax[:q], phase_ms=[float(v) for v in ms])

    # ---- a roadmap planted from the host; the roadmap re-checked against the current obstacles

    def set_roadmap(self, states, offsets, neighbours):
        """Replaces the roadmap with (states [n][dim], offsets [n+1], neighbours [E]), the layout roadmap() returns.  The
        structure is checked on the device; a violation raises OxhipError(ERR_BAD_ARG) naming the rule and the lowest
        offending row, and leaves the handle as it was."""
        off = np.ascontiguousarray(np.asarray(offsets).reshape(-1), dtype=np.uint64)
        n = off.size - 1
        if n < 0:
            raise OxhipError(ERR_BAD_ARG, "offsets must hold n + 1 entries")
        s = _f64(states).reshape(-1)
        if s.size != n * self.dim:
            raise OxhipError(ERR_BAD_ARG, "states must be [n][dim] for offsets of n + 1 entries")
        if s.size == 0:
            s = np.zeros(1, dtype=np.float64)
        nb = np.ascontiguousarray(np.asarray(neighbours).reshape(-1), dtype=np.uint32)
        _check(lib().oxhip_prm_set_roadmap(self._h, _p(s), n, _p(off, _u64p), _p(nb, _u32p) if nb.size else None))

    def revalidate(self):
        """Re-checks every milestone and every edge against the obstacles as they are now.  Returns (valid_mask [n] bool,
        n_removed_entries); an invalid milestone keeps its index and loses its entries."""
        n = self.sizes()[0]
        valid = np.zeros(max(n, 1), dtype=np.uint8)
        removed = C.c_uint64()
        _check(lib().oxhip_prm_revalidate(self._h, _p(valid, _u8p), None, C.byref(removed)))   # (the invalid count is the mask's zeros)
        return valid[:n].astype(bool), removed.value

    def revalidate_last_timing(self):
        """dict(phase_ms=[milestone validity, pair emission, edge checks, compaction]) of the last revalidate"""
        return dict(phase_ms=_phase_ms(lib().oxhip_prm_revalidate_last_timing, self._h, 4).tolist())

    # ---- the roadmap grown in place

    def grow(self, n_more, max_samples=0, new_stream=None):
        """Adds up to n_more milestones to the roadmap as it stands, under the obstacles as they are now (oxhip_prm_grow_roadmap).
        new_stream=None continues the handle's own sampler stream where construct_roadmap / the last grow stopped;
        new_stream=id starts stream `id` at its first word (what a planted roadmap needs).  max_samples=0 is construct's rule.
        Returns (n_added, n_samples_drawn)."""
        g = PrmGrowConfig()
        g.struct_size = C.sizeof(PrmGrowConfig)
        g.n_more, g.max_samples = n_more, max_samples
        if new_stream is not None:
            g.flags, g.stream = PRM_GROW_NEW_STREAM, new_stream
        added, drawn = C.c_uint32(), C.c_uint64()
        _check(lib().oxhip_prm_grow_roadmap(self._h, C.byref(g), C.byref(added), C.byref(drawn)))
        return added.value, drawn.value

    def grow_timing(self):
        """dict(phase_ms=[liveness mask, keys from CSR, sample, pairs (+ filter), edges, sort + CSR]) of the last grow"""
        return dict(phase_ms=_phase_ms(lib().oxhip_prm_grow_last_timing, self._h, 6).tolist())

    # ---- the roadmap as a graph: connected components, and pruning

    def components(self):
        """(label [n] u32, size [n] u32, n_components, largest_label, largest_size): label[i] is the lowest milestone index of
        i's connected component, size[i] its number of milestones; the largest component's ties go to the lowest label.  Only
        the CSR is read; a row without entries is a component of its own (oxhip_prm_components)."""
        n = self.sizes()[0]
        label, size = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
        nc, ll, ls = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(lib().oxhip_prm_components(self._h, _p(label, _u32p), _p(size, _u32p), n, C.byref(nc), C.byref(ll), C.byref(ls)))
        return label[:n], size[:n], nc.value, ll.value, ls.value

    def components_timing(self):
        """dict(phase_ms=[init + hook, flatten, sizes + summary, copies], launches) of the last components()"""
        launches = C.c_uint32()
        ms = _phase_ms(lib().oxhip_prm_components_last_timing, self._h, 4, launches)
        return dict(phase_ms=ms.tolist(), launches=launches.value)

    def prune(self, invalid=False, keep=None, min_size=0, largest=False):
        """Removes milestones and renumbers the rest, order kept (oxhip_prm_prune).  Stage 1: invalid=True drops the milestones
        that are invalid now, keep=[n] bools drops those with a false entry.  Stage 2, on the components of what stage 1 left:
        min_size > 0 drops components with fewer milestones, largest=True keeps only the largest component.  Not a re-check:
        no edge is tested.  Returns (new_index [n before] i32 with -1 = dropped, n_kept, n_removed_entries)."""
        n = self.sizes()[0]
        c = PrmPruneConfig()
        c.struct_size = C.sizeof(PrmPruneConfig)
        c.flags = ((PRM_PRUNE_INVALID if invalid else 0) | (PRM_PRUNE_MASK if keep is not None else 0)
                   | (PRM_PRUNE_MIN_SIZE if min_size else 0) | (PRM_PRUNE_LARGEST if largest else 0))
        c.min_size = min_size
        mask = None
        if keep is not None:
            mask = np.ascontiguousarray(np.asarray(keep).reshape(-1) != 0, dtype=np.uint8)
            if mask.size != n:
                raise OxhipError(ERR_BAD_ARG, "keep must hold one entry per milestone")
            if mask.size == 0:
                mask = np.zeros(1, dtype=np.uint8)
        new_index = np.zeros(max(n, 1), dtype=np.int32)
        kept, removed = C.c_uint32(), C.c_uint64()
        _check(lib().oxhip_prm_prune(self._h, C.byref(c), None if mask is None else _p(mask, _u8p), _p(new_index, _i32p),
                                     C.byref(kept), C.byref(removed)))
        return new_index[:n], kept.value, removed.value

    def prune_timing(self):
        """dict(phase_ms=[masks, components, scans, move entries, move states]) of the last prune"""
        return dict(phase_ms=_phase_ms(lib().oxhip_prm_prune_last_timing, self._h, 5).tolist())

    # ---- the handle's own checker; the last batch's paths subdivided and shortcut on the device

    def is_valid(self, states):
        """the handle's StateValidityChecker over rows [n][dim], against the obstacles as they are now -> [n] bool"""
        s = _f64(states).reshape(-1, self.dim)
        out = np.empty(max(s.shape[0], 1), dtype=np.uint8)
        _check(lib().oxhip_prm_is_valid(self._h, _p(s if s.size else np.zeros(1)), s.shape[0], _p(out, _u8p)))
        return out[:s.shape[0]].astype(bool)

    def check_motion(self, frm, to):
        """the check_motion that construction uses, from[i] -> to[i] -> [n] bool"""
        a = _f64(frm).reshape(-1, self.dim)
        b = _f64(to, a.shape)
        out = np.empty(max(a.shape[0], 1), dtype=np.uint8)
        pad = np.zeros(1)
        _check(lib().oxhip_prm_check_motion(self._h, _p(a if a.size else pad), _p(b if b.size else pad), a.shape[0], _p(out, _u8p)))
        return out[:a.shape[0]].astype(bool)

    def simplify_batch_paths(self, subdivide=1, max_span=0, chunk_queries=0):
        """Shortcut every answered path of the last batch, each edge first cut into `subdivide` equal parts
        (include/oxmpl_hip.h states the semantics).  max_span bounds a link in original edges, 0 = no bound.  chunk_queries:
        queries per device round (test-only; results never depend on it)."""
        _check(lib().oxhip_prm_batch_simplify_paths(self._h, int(subdivide), int(max_span), int(chunk_queries)))

    def simplified_batch_paths(self):
        """(offsets [Q+1] u64, states [rows][dim], indices [rows] u32 into the dense path) of the last simplify_batch_paths"""
        offsets = np.zeros(getattr(self, "_batch_q", 0) + 1, dtype=np.uint64)
        states, idx = _sized(lib().oxhip_prm_batch_get_simplified_paths, (self._h, _p(offsets, _u64p)),
                             [(np.float64, self.dim), (np.uint32, 0)], C.c_uint64)
        return offsets, states, idx

    def simplify_results(self):
        """dict(raw_cost [Q], simplified_cost [Q], checks [Q] u64) of the last simplify_batch_paths"""
        q = getattr(self, "_batch_q", 0)
        raw, simp, checks = np.zeros(max(q, 1)), np.zeros(max(q, 1)), np.zeros(max(q, 1), dtype=np.uint64)
        _check(lib().oxhip_prm_batch_get_simplify_results(self._h, _p(raw), _p(simp), _p(checks, _u64p)))
        return dict(raw_cost=raw[:q], simplified_cost=simp[:q], checks=checks[:q])

    def batch_path_valid_matrix(self, query, subdivide=1, max_span=0):
        """test hook: valid(u, v) of query `query`'s dense path as the pair kernel evaluates it, [M][M] bool (u < v; same-edge
        pairs read True)"""
        out, = _sized(lib().oxhip_prm_batch_path_valid_matrix, (self._h, int(query), int(subdivide), int(max_span)), [(np.uint8, 0)],
                      capacity=lambda M: M * M, fill_empty=False)   # the count is the dense length M, the buffer holds M * M verdicts
        M = math.isqrt(out.size)
        return out.reshape(M, M).astype(bool)

    def simplify_timing(self):
        """dict(phase_ms=[upload + subdivide, pair matrix, DP, copies], rounds) of the last simplify_batch_paths"""
        r = C.c_uint32()
        ms = _phase_ms(lib().oxhip_prm_batch_simplify_last_timing, self._h, 4, r)
        return dict(phase_ms=ms.tolist(), rounds=r.value)
