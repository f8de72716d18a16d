"""Writes tests/golden/prm_create_refusals.json: what oxhip_prm_create answers, before it chooses a device, to configs it
refuses and to configs it accepts.

One record per refusal that precedes select_device in oxhip_prm_create, records that break two rules at once (each pins an
adjacent pair of the order of the checks), and records that pass validation: on the machine that writes the file -- it has no
GPU -- those end with OXHIP_ERR_NO_DEVICE.  A record holds every field of oxhip_prm_config (doubles as hex floats), the status
code and oxhip_last_error_string.  The config goes through ctypes as a raw struct, so any field can be set, struct_size included.

The file is a record of the library BEFORE a change to oxhip_prm_create: build the commit to be pinned, run this against it and
name the commit, then replay the file against the changed library (tests/test_prm_create_refusals.py).

    OXMPL_HIP_LIB=<that commit's liboxmpl_hip.so> python tests/golden/make_golden_prm_create_refusals.py <commit>
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
DOUBLES = ("timeout", "connection_radius", "lvs_fraction")
BASE = dict(struct_size=C.sizeof(capi.PrmConfig), dim=2, bounds=[0.0, 10.0, 0.0, 10.0], timeout=0.0, connection_radius=1.5,
            lvs_fraction=0.05, max_milestones=100, device=0, max_samples=0, seed=42, stream=0, knn_k=0,
            space=capi.SPACE_REAL_VECTOR)
SO3 = dict(space=capi.SPACE_SO3, dim=4, bounds=[0.0, 0.0, 0.0, 1.0, PI], connection_radius=0.5)


def _with(base, **kw):
    d = dict(base)
    d.update(kw)
    return d


def _b(base, **kw):   # the bounds of `base` with entries replaced: _b(SO3, b4=-0.25)
    b = list(base["bounds"])
    for k, v in kw.items():
        b[int(k[1:])] = v
    return b


# (name, overrides of BASE); in the order of the checks in oxhip_prm_create
CASES = [
    ("struct_size_short", dict(struct_size=C.sizeof(capi.PrmConfig) - 8)),
    ("struct_size_zero", dict(struct_size=0)),
    ("no_milestones", dict(max_milestones=0)),
    ("max_milestones_too_large", dict(max_milestones=(1 << 26) + 1)),
    ("radius_nan", dict(connection_radius=NAN)),
    ("space_unknown", dict(space=4)),
    ("space_se2", dict(space=capi.SPACE_SE2)),
    ("space_se3", dict(space=capi.SPACE_SE3, dim=7)),
    # R^n
    ("rn_dim_zero", dict(dim=0)),
    ("rn_dim_nine", dict(dim=9)),
    ("rn_unbounded", dict(bounds=[0.0, INF, 0.0, 10.0])),
    ("rn_unbounded_second_axis", dict(bounds=[0.0, 10.0, NAN, 10.0])),
    ("rn_zero_volume", dict(bounds=[0.0, 10.0, 3.0, 3.0])),
    ("rn_bounds_beyond_1e150", dict(bounds=[0.0, 10.0, 0.0, 1e151])),
    ("rn_fraction_zero", dict(lvs_fraction=0.0)),
    ("rn_fraction_negative", dict(lvs_fraction=-1.0)),
    ("rn_1e6_checks_by_fraction", dict(lvs_fraction=1e-9)),
    ("rn_1e6_checks_by_radius", dict(connection_radius=1e9)),
    # SO(3)
    ("so3_dim", _with(SO3, dim=3)),
    ("so3_centre_nan", _with(SO3, bounds=_b(SO3, b1=NAN))),
    ("so3_centre_inf", _with(SO3, bounds=_b(SO3, b3=INF))),
    ("so3_max_angle_negative", _with(SO3, bounds=_b(SO3, b4=-1e-300))),
    ("so3_fraction_zero", _with(SO3, lvs_fraction=-1.0)),
    ("so3_1e6_checks_by_extent", _with(SO3, lvs_fraction=1e-6)),
    ("so3_knn", _with(SO3, knn_k=4)),
    # (0.5 PI / res <= 1e6 has passed by then, so min(radius, PI / 2) / res > 1e6 cannot hold: see _unreachable)
    # two rules broken at once: the earlier check answers
    ("order_struct_size_and_milestones", dict(struct_size=16, max_milestones=0)),
    ("order_milestones_and_radius", dict(max_milestones=0, connection_radius=NAN)),
    ("order_radius_and_space", dict(connection_radius=NAN, space=9)),
    ("order_space_and_dim", dict(space=9, dim=0)),
    ("order_rn_dim_and_unbounded", dict(dim=9, bounds=[0.0, INF, 0.0, 10.0])),
    ("order_rn_unbounded_and_zero_volume", dict(bounds=[INF, -INF, 0.0, 10.0])),
    ("order_rn_zero_volume_and_beyond", dict(bounds=[1e151, 1e151, 0.0, 10.0])),
    ("order_rn_first_axis_beyond_and_second_unbounded", dict(bounds=[0.0, 1e151, 0.0, INF])),
    ("order_rn_beyond_and_fraction", dict(bounds=[0.0, 10.0, -1e200, 10.0], lvs_fraction=0.0)),
    ("order_rn_fraction_and_1e6_checks", dict(lvs_fraction=0.0, connection_radius=1e300)),
    ("order_so3_dim_and_centre", _with(SO3, dim=5, bounds=_b(SO3, b0=INF))),
    ("order_so3_centre_and_max_angle", _with(SO3, bounds=_b(SO3, b2=NAN, b4=-1.0))),
    ("order_so3_max_angle_and_fraction", _with(SO3, bounds=_b(SO3, b4=-1.0), lvs_fraction=0.0)),
    ("order_so3_fraction_and_knn", _with(SO3, lvs_fraction=0.0, knn_k=1)),
    ("order_so3_1e6_checks_and_knn", _with(SO3, lvs_fraction=1e-7, knn_k=1)),
    # configs that pass validation: the answer is about the device
    ("ok_r2_radius", dict()),
    ("ok_r3_knn", dict(dim=3, bounds=[0.0, 10.0] * 3, knn_k=4)),
    ("ok_r8_knn_radius_inf", dict(dim=8, bounds=[-1.0, 1.0] * 8, knn_k=8, connection_radius=INF)),
    ("ok_radius_inf", dict(connection_radius=INF)),
    ("ok_radius_zero", dict(connection_radius=0.0)),
    ("ok_radius_negative", dict(connection_radius=-1.0)),
    ("ok_fraction_clamped", dict(lvs_fraction=7.0)),
    ("ok_fraction_nan", dict(lvs_fraction=NAN)),
    ("ok_so3", SO3),
    ("ok_so3_radius_inf", _with(SO3, connection_radius=INF)),
    ("ok_so3_radius_negative", _with(SO3, connection_radius=-0.5)),
    ("ok_so3_max_angle_nan", _with(SO3, bounds=_b(SO3, b4=NAN))),
]


def fields_of(overrides):
    f = _with(BASE, **overrides)
    f["bounds"] = [float(v).hex() for v in list(f["bounds"]) + [0.0] * (2 * capi.MAX_DIM - len(f["bounds"]))]
    for k in DOUBLES:
        f[k] = float(f[k]).hex()
    return f


def config_of(fields):
    """the ctypes struct of a record's fields (the test replays records through this, too)"""
    cfg = capi.PrmConfig()
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
    st = lib.oxhip_prm_create(None if null == "cfg" else C.byref(cfg), None if null == "out" else C.byref(h))
    msg = lib.oxhip_last_error_string().decode() if st != capi.OK else ""
    if h.value:
        lib.oxhip_prm_destroy(h)
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
    head = {"_generator": "tests/golden/make_golden_prm_create_refusals.py", "_library_commit": commit,
            "_unreachable": ["SO(3): min(connection_radius, PI / 2) / res > 1e6 (so3_space_resolution has refused 0.5 PI / res > 1e6 "
                             "by then, and min(r, PI / 2) <= 0.5 PI with the same res; a NaN radius was refused earlier)"]}
    path = os.path.join(HERE, "prm_create_refusals.json")
    with open(path, "w") as f:   # one record per line
        f.write(json.dumps(head, separators=(",", ":"))[:-1] + ',"records":[\n')
        f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in records) + "\n]}\n")
    print("wrote", path, len(records), "records,", len({r["message"] for r in records}), "distinct messages")


if __name__ == "__main__":
    main()
