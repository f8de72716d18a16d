"""Writes tests/golden/rrt_create_refusals.json: what oxhip_rrt_batch_create answers, before it chooses a device, to configs it
refuses and to configs it accepts.

One record per refusal that precedes select_device in create(), records that break two rules at once (they pin the order of
the checks), and records that pass validation: on the machine that writes the file -- it has no GPU -- those end with
OXHIP_ERR_NO_DEVICE.  A record holds every field of oxhip_rrt_config (doubles as hex floats), the status code and
oxhip_last_error_string.  The config goes through ctypes as a raw struct, so any field can be set, struct_size included.

The file is a record of the library BEFORE a change to create(): build the commit to be pinned, run this against it and name
the commit, then replay the file against the changed library (tests/test_create_refusals.py).

    OXMPL_HIP_LIB=<that commit's liboxmpl_hip.so> python tests/golden/make_golden_create_refusals.py <commit>
"""
import ctypes as C
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oxmpl_amd import capi  # noqa: E402

INF, NAN, PI = math.inf, math.nan, math.pi
DOUBLES = ("max_distance", "goal_bias", "lvs_fraction", "search_radius")
BASE = dict(struct_size=C.sizeof(capi.Config), dim=2, bounds=[0.0, 10.0, 0.0, 10.0], max_distance=0.5, goal_bias=0.05,
            lvs_fraction=0.05, n_problems=2, max_nodes=100, stop_at_goal=1, kernel=capi.KERNEL_AUTO, seed=42, first_problem_id=0,
            device=0, planner=capi.PLANNER_RRT, search_radius=0.0, space=capi.SPACE_REAL_VECTOR,
            goal_sampler=capi.GOAL_SAMPLE_CENTRE, debug_flags=0, star_pool_share=0, frozen_split=0, reserved=0)
CONNECT, STAR = capi.PLANNER_RRT_CONNECT, capi.PLANNER_RRT_STAR
SE2 = dict(space=capi.SPACE_SE2, dim=3, planner=CONNECT, bounds=[0.0, 10.0, 0.0, 10.0, -PI, PI])
SO3 = dict(space=capi.SPACE_SO3, dim=4, bounds=[0.0, 0.0, 0.0, 1.0, PI])
SE3 = dict(space=capi.SPACE_SE3, dim=7, planner=CONNECT, bounds=[-5.0, 5.0] * 3 + [0.0, 0.0, 0.0, 1.0, PI])


def _with(base, **kw):
    d = dict(base)
    d.update(kw)
    return d


def _b(base, **kw):   # the bounds of `base` with entries replaced: _b(SE3, b10=-0.25)
    b = list(base["bounds"])
    for k, v in kw.items():
        b[int(k[1:])] = v
    return b


# (name, overrides of BASE); in the order of the checks in create()
CASES = [
    ("struct_size_short", dict(struct_size=C.sizeof(capi.Config) - 8)),
    ("struct_size_zero", dict(struct_size=0)),
    ("dim_zero", dict(dim=0)),
    ("dim_nine", dict(dim=9)),
    ("no_problems", dict(n_problems=0)),
    ("no_nodes", dict(max_nodes=0)),
    ("max_nodes_too_large", dict(max_nodes=(1 << 30) + 1)),
    ("goal_bias_negative", dict(goal_bias=-0.1)),
    ("goal_bias_above_one", dict(goal_bias=1.5)),
    ("goal_bias_nan", dict(goal_bias=NAN)),
    ("max_distance_zero", dict(max_distance=0.0)),
    ("max_distance_inf", dict(max_distance=INF)),
    ("max_distance_nan", dict(max_distance=NAN)),
    ("kernel_unknown", dict(kernel=7)),
    ("kernel_retired_3", dict(kernel=3)),
    ("kernel_retired_4", dict(kernel=4)),
    ("planner_unknown", dict(planner=3)),
    ("frozen_split_65", dict(frozen_split=65)),
    ("connect_on_cells", dict(planner=CONNECT, kernel=capi.KERNEL_CELLS)),
    ("connect_on_resident", dict(planner=CONNECT, kernel=capi.KERNEL_RESIDENT)),
    ("connect_on_lanes", dict(planner=CONNECT, kernel=capi.KERNEL_LANES)),
    ("star_on_resident", dict(planner=STAR, kernel=capi.KERNEL_RESIDENT, search_radius=1.0)),
    ("star_radius_nan", dict(planner=STAR, search_radius=NAN)),
    ("goal_sampler_unknown", dict(goal_sampler=2)),
    ("disc_in_r3", dict(goal_sampler=1, dim=3, bounds=[0.0, 10.0] * 3)),
    ("disc_in_so3", _with(SO3, goal_sampler=1)),
    ("disc_in_se3", _with(SE3, goal_sampler=1)),
    ("disc_with_connect", dict(goal_sampler=1, planner=CONNECT)),
    ("disc_on_resident", dict(goal_sampler=1, kernel=capi.KERNEL_RESIDENT)),
    ("space_unknown", dict(space=4)),
    # SE(3)
    ("se3_dim", _with(SE3, dim=6)),
    ("se3_planner_rrt", _with(SE3, planner=capi.PLANNER_RRT)),
    ("se3_planner_star", _with(SE3, planner=STAR, search_radius=1.0)),
    ("se3_kernel_lanes", _with(SE3, kernel=capi.KERNEL_LANES)),
    ("se3_unbounded", _with(SE3, bounds=_b(SE3, b3=INF))),
    ("se3_zero_volume", _with(SE3, bounds=_b(SE3, b4=5.0))),
    ("se3_bounds_beyond_1e150", _with(SE3, bounds=_b(SE3, b0=-1e200))),
    ("se3_fraction_zero", _with(SE3, lvs_fraction=0.0)),
    ("se3_centre_not_finite", _with(SE3, bounds=_b(SE3, b8=INF))),
    ("se3_max_angle_negative", _with(SE3, bounds=_b(SE3, b10=-0.25))),
    ("se3_1e6_checks", _with(SE3, lvs_fraction=1e-9)),
    # SO(3)
    ("so3_dim", _with(SO3, dim=3)),
    ("so3_planner_connect", _with(SO3, planner=CONNECT)),
    ("so3_planner_star", _with(SO3, planner=STAR, search_radius=1.0)),
    ("so3_kernel_lanes", _with(SO3, kernel=capi.KERNEL_LANES)),
    ("so3_kernel_cells", _with(SO3, kernel=capi.KERNEL_CELLS)),
    ("so3_centre_nan", _with(SO3, bounds=_b(SO3, b1=NAN))),
    ("so3_max_angle_negative", _with(SO3, bounds=_b(SO3, b4=-1e-300))),
    ("so3_fraction_zero", _with(SO3, lvs_fraction=-1.0)),
    ("so3_1e6_checks", _with(SO3, lvs_fraction=1e-6)),
    # SE(2)
    ("se2_dim", _with(SE2, dim=2)),
    ("se2_planner_rrt", _with(SE2, planner=capi.PLANNER_RRT)),
    ("se2_theta_empty", _with(SE2, bounds=_b(SE2, b4=1.0, b5=1.0))),
    ("se2_theta_nan", _with(SE2, bounds=_b(SE2, b4=NAN))),
    ("se2_unbounded", _with(SE2, bounds=_b(SE2, b0=-INF))),
    ("se2_zero_volume", _with(SE2, bounds=_b(SE2, b2=10.0))),
    ("se2_fraction_zero", _with(SE2, lvs_fraction=0.0)),
    ("se2_1e6_checks", _with(SE2, lvs_fraction=1e-9)),
    # R^n
    ("rn_unbounded", dict(bounds=[0.0, INF, 0.0, 10.0])),
    ("rn_unbounded_second_axis", dict(bounds=[0.0, 10.0, NAN, 10.0])),
    ("rn_zero_volume", dict(bounds=[0.0, 10.0, 3.0, 3.0])),
    ("rn_bounds_beyond_1e150", dict(bounds=[0.0, 10.0, 0.0, 1e151])),
    ("rn_fraction_zero", dict(lvs_fraction=0.0)),
    ("rn_1e6_checks", dict(lvs_fraction=1e-9)),
    ("rn_1e6_checks_by_max_distance", dict(max_distance=1e9)),
    # two rules broken at once: the earlier check answers
    ("order_space_unknown_and_dim", dict(space=9, dim=0)),
    ("order_space_unknown_and_bounds", dict(space=9, bounds=[0.0, INF, 0.0, 10.0])),
    ("order_se3_planner_and_max_angle", _with(SE3, planner=capi.PLANNER_RRT, bounds=_b(SE3, b10=-0.25))),
    ("order_se3_dim_and_planner", _with(SE3, dim=4, planner=capi.PLANNER_RRT)),
    ("order_se3_bounds_and_max_angle", _with(SE3, bounds=_b(SE3, b1=INF, b10=-0.25))),
    ("order_so3_planner_and_kernel", _with(SO3, planner=CONNECT, kernel=capi.KERNEL_LANES)),
    ("order_so3_kernel_and_centre", _with(SO3, kernel=capi.KERNEL_CELLS, bounds=_b(SO3, b0=INF))),
    ("order_se2_theta_and_xy", _with(SE2, bounds=_b(SE2, b0=INF, b4=2.0, b5=1.0))),
    ("order_se2_dim_and_planner", _with(SE2, dim=4, planner=STAR)),
    ("order_struct_size_and_dim", dict(struct_size=16, dim=0)),
    ("order_goal_bias_and_max_distance", dict(goal_bias=2.0, max_distance=-1.0)),
    ("order_kernel_and_planner", dict(kernel=9, planner=9)),
    ("order_retired_kernel_and_frozen_split", dict(kernel=3, frozen_split=100)),
    ("order_connect_cells_and_space", dict(planner=CONNECT, kernel=capi.KERNEL_CELLS, space=7)),
    ("order_disc_and_space_unknown", dict(goal_sampler=1, space=5)),
    ("order_star_radius_and_sampler", dict(planner=STAR, search_radius=NAN, goal_sampler=3)),
    ("order_bounds_and_1e6_checks", dict(bounds=[0.0, 10.0, 5.0, 1.0], max_distance=1e12)),
    # configs that pass validation: the answer is about the device
    ("ok_r2_rrt", dict()),
    ("ok_r2_rrt_cells", dict(kernel=capi.KERNEL_CELLS)),
    ("ok_r8_stream", dict(dim=8, bounds=[-1.0, 1.0] * 8, kernel=capi.KERNEL_STREAM)),
    ("ok_r3_connect", dict(dim=3, bounds=[0.0, 10.0] * 3, planner=CONNECT)),
    ("ok_r3_star", dict(dim=3, bounds=[0.0, 10.0] * 3, planner=STAR, search_radius=1.0)),
    ("ok_r2_disc", dict(goal_sampler=1)),
    ("ok_fraction_clamped", dict(lvs_fraction=7.0)),
    ("ok_fraction_nan", dict(lvs_fraction=NAN)),
    ("ok_se2", SE2),
    ("ok_se2_theta_clamped", _with(SE2, bounds=_b(SE2, b4=-9.0, b5=9.0))),
    ("ok_so3", SO3),
    ("ok_so3_max_angle_nan", _with(SO3, bounds=_b(SO3, b4=NAN), kernel=capi.KERNEL_STREAM)),
    ("ok_se3", SE3),
    ("ok_se3_stream", _with(SE3, kernel=capi.KERNEL_STREAM)),
]


def fields_of(overrides):
    f = _with(BASE, **overrides)
    f["bounds"] = [float(v).hex() for v in list(f["bounds"]) + [0.0] * (2 * capi.MAX_DIM - len(f["bounds"]))]
    for k in DOUBLES:
        f[k] = float(f[k]).hex()
    return f


def config_of(fields):
    """the ctypes struct of a record's fields (the test replays records through this, too)"""
    cfg = capi.Config()
    for k, v in fields.items():
        if k == "bounds":
            for i, h in enumerate(v):
                cfg.bounds[i] = float.fromhex(h)
        else:
            setattr(cfg, k, float.fromhex(v) if k in DOUBLES else v)
    return cfg


def create(lib, fields, null=None):
    """(status, oxhip_last_error_string); destroys what an accepted config created"""
    cfg, h = config_of(fields), C.c_void_p()
    st = lib.oxhip_rrt_batch_create(None if null == "cfg" else C.byref(cfg), None if null == "out" else C.byref(h))
    msg = lib.oxhip_last_error_string().decode() if st != capi.OK else ""
    if h.value:
        lib.oxhip_rrt_batch_destroy(h)
    return st, msg


def main():
    commit = sys.argv[1]
    lib = capi.lib()
    n = C.c_int32()
    assert lib.oxhip_device_count(C.byref(n)) == capi.ERR_NO_DEVICE, "write this file on a machine without a GPU"
    records = []
    for null in ("cfg", "out"):
        st, msg = create(lib, fields_of({}), null)
        records.append(dict(name="null_" + null, null=null, fields=fields_of({}), code=st, message=msg))
    for name, overrides in CASES:
        f = fields_of(overrides)
        st, msg = create(lib, f)
        assert (st == capi.ERR_NO_DEVICE) == name.startswith("ok_"), (name, st, msg)
        records.append(dict(name=name, null=None, fields=f, code=st, message=msg))
    assert len({r["name"] for r in records}) == len(records)
    head = {"_generator": "tests/golden/make_golden_create_refusals.py", "_library_commit": commit,
            "_unreachable": ["SE(3): the goal sampler must be OXHIP_GOAL_SAMPLE_CENTRE (the disc sampler's own check answers first)",
                             "SE(3) RRTConnect runs on rrt_connect_se3.hip: kernel must be ... (RRTConnect's own kernel check answers first)",
                             "dim must be in 1..8 / SO(3) dim must be 4 inside the resolution helpers (create checks both earlier)"]}
    path = os.path.join(HERE, "rrt_create_refusals.json")
    with open(path, "w") as f:   # one record per line
        f.write(json.dumps(head, separators=(",", ":"))[:-1] + ',"records":[\n')
        f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in records) + "\n]}\n")
    print("wrote", path, len(records), "records,", len({r["message"] for r in records}), "distinct messages")


if __name__ == "__main__":
    main()
