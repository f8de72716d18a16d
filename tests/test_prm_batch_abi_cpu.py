"""CPU: the batched-query additions to the PRM ABI (oxhip_prm_solve_batch and the four oxhip_prm_batch_* getters, prm_batch.hip).
(i)   header, capi.EXPORTS, the library and rust/oxmpl-hip/src/ffi.rs agree on the five names and their arity; the ABI version
      and both configuration structs are what they were;
(ii)  null handles and null pointers are OXHIP_ERR_BAD_ARG;
(iii) without a device the Python mirror reaches ERR_NO_DEVICE at setup, not earlier, and solve_batch before setup() is the
      reference's "uninitialised" message;
(iv)  prm_batch.hip compiles for gfx950 without scratch, VGPR spills or flat / scratch memory instructions; the search kernel
      takes its parents with an integer atomic minimum and holds no 64-bit floating-point instruction;
(v)   the oracle (oracle/prm_oracle.c) answers the R^n scenes of tests/golden/prm_batch_golden.json as recorded."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import unhex, bits
from prm_helpers import make_oracle_prm, STATUS_NAME
from oxmpl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oxmpl_amd", "csrc")
NEW = {"oxhip_prm_solve_batch": 8, "oxhip_prm_batch_get_results": 6, "oxhip_prm_batch_get_paths": 6,
       "oxhip_prm_batch_get_query_sets": 8, "oxhip_prm_batch_last_timing": 3}


@pytest.fixture(scope="module")
def L():
    capi.build_library()
    return capi.lib()


def _arity(text, name, opener):
    m = re.search(re.escape(opener + name) + r"\s*\(([^;{]*?)\)\s*(?:->\s*i32)?\s*;", text, re.S)
    assert m, name
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return len([a for a in args.split(",") if a.strip()])


def test_header_exports_library_and_rust_agree(L):
    header = open(os.path.join(ROOT, "include", "oxmpl_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "oxmpl-hip", "src", "ffi.rs")).read()
    for name, arity in NEW.items():
        assert name in capi.EXPORTS and hasattr(L, name)
        assert _arity(header, name, "int32_t ") == arity, name
        assert _arity(ffi, name, "pub fn ") == arity, name
        assert len(getattr(L, name).argtypes) == arity and getattr(L, name).restype is C.c_int32
    assert capi.ABI_VERSION == 2 and L.oxhip_abi_version() == 2
    assert re.search(r"#define\s+OXHIP_ABI_VERSION\s+2\b", header)
    assert C.sizeof(capi.Config) == 232 and C.sizeof(capi.PrmConfig) == 200


def test_null_handles_and_pointers_are_bad_arg(L):
    d, i32, u32, u64 = (C.c_double * 8)(), (C.c_int32 * 2)(), (C.c_uint32 * 2)(), (C.c_uint64 * 3)()
    assert L.oxhip_prm_solve_batch(None, 1, d, d, d, 0.0, 0, i32) == capi.ERR_BAD_ARG
    assert L.oxhip_prm_solve_batch(None, 0, None, None, None, 0.0, 0, None) == capi.ERR_BAD_ARG
    assert L.oxhip_prm_batch_get_results(None, i32, u32, i32, u32, u32) == capi.ERR_BAD_ARG
    assert L.oxhip_prm_batch_get_paths(None, u64, u32, d, 1, u64) == capi.ERR_BAD_ARG
    assert L.oxhip_prm_batch_get_query_sets(None, 0, u32, 2, u32, u32, 2, u32) == capi.ERR_BAD_ARG
    assert L.oxhip_prm_batch_last_timing(None, d, u32) == capi.ERR_BAD_ARG
    assert b"null" in L.oxhip_last_error_string()


def test_python_mirror_without_a_device(L):
    from oxmpl_amd.base import ProblemDefinition, RealVectorState, RealVectorStateSpace, SphereBoxValidityChecker
    from oxmpl_amd.geometric import PRM, _MESSAGES

    class Goal:
        def __init__(self, target, radius):
            self.target, self.radius = target, radius

    space = RealVectorStateSpace(2, [(0.0, 10.0), (0.0, 10.0)])
    pd = ProblemDefinition(space, RealVectorState([1.0, 5.0]), Goal(RealVectorState([9.0, 5.0]), 0.5))
    planner = PRM(5.0, 0.5, pd, max_milestones=100)
    with pytest.raises(Exception) as ei:       # prm.rs:229-236
        planner.solve_batch([pd, pd], 1.0)
    assert str(ei.value) == _MESSAGES[capi.ERR_PLANNER_UNINITIALISED]
    n = C.c_int32()
    if L.oxhip_device_count(C.byref(n)) == capi.OK:
        return                                  # (the rest is about a machine without a device)
    with pytest.raises(capi.OxhipError) as ei:
        planner.setup(SphereBoxValidityChecker(boxes=[([4.75, 2.0], [5.25, 8.0])]))
    assert ei.value.status == capi.ERR_NO_DEVICE
    with pytest.raises(capi.OxhipError) as ei:
        capi.PRMRoadmap(2, [(0.0, 10.0), (0.0, 10.0)], 0.5, 100)
    assert ei.value.status == capi.ERR_NO_DEVICE


def _kernels(asm):
    """name -> (metadata, instructions of the body)"""
    meta = {}
    for block in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|"
                                                        r"group_segment_fixed_size|max_flat_workgroup_size):\s+(\d+)", block)}
    out = {}
    for name, m in meta.items():
        body = asm.split("\n" + name + ":")[1].split(".Lfunc_end")[0]
        out[name] = (m, body)
    return out


def test_prm_batch_kernels_resource_shape(tmp_path):
    out = str(tmp_path / "prm_batch.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                           "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "prm_batch.hip")], stderr=subprocess.DEVNULL)
    kernels = _kernels(open(out).read())
    names = sorted(kernels)
    assert sum("prm_batch_flags_kernel" in k for k in names) == 9          # dim 1 .. 8, and DIM = 0:
    assert sum("prm_batch_flags_kernelILi0E" in k for k in names) == 1     # SO(3)
    assert sum("prm_batch_search_kernel" in k for k in names) == 10        # 4, 8, 16, 32, 64 lanes per level node x visited bits in LDS or not
    assert sum("prm_batch_paths_kernel" in k for k in names) == 1
    assert len(names) == 20
    for name, (m, body) in kernels.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert "flat_load" not in body and "flat_store" not in body and "scratch_" not in body, name
        assert len(body) > 200, name
        if "search_kernel" in name:
            assert m["max_flat_workgroup_size"] == 1024 and m["group_segment_fixed_size"] <= 256, (name, m)
            assert "global_atomic_umin" in body and "ds_min_u32" in body, name     # the claims; the lowest-ranked goal of a level
            assert not re.search(r"_f64|_f32|_f16", body), name                    # integer decisions only
        if "flags_kernel" in name:
            assert "v_mul_f64" in body and "v_add_f64" in body, name   # binary64 geometry (fma only inside sqrt / division sequences)


@pytest.mark.parametrize("scene", ["wall", "r6"])
def test_oracle_answers_the_batch_golden_queries(scene):
    with open(os.path.join(ROOT, "tests", "golden", "prm_batch_golden.json")) as f:
        rec = json.load(f)[scene]
    with open(os.path.join(ROOT, "tests", "golden", "prm_golden.json")) as f:
        P = json.load(f)[scene]["params"]
    qs = rec["queries"]
    assert len(qs) == 32 and rec["space"] == "real_vector"
    o = make_oracle_prm(P)
    o.setup([unhex(v) for v in qs[0]["start"]], [unhex(v) for v in qs[0]["goal_c"]], unhex(qs[0]["goal_r"]))
    o.construct_roadmap(P["max_milestones"], P["max_samples"])
    assert o.num_milestones == rec["n"]
    states = o.roadmap()[0]
    seen = set()
    for k, q in enumerate(qs):
        o.set_problem([unhex(v) for v in q["start"]], [unhex(v) for v in q["goal_c"]], unhex(q["goal_r"]))
        st = o.solve()
        assert STATUS_NAME[st] == q["status"], k
        seen.add(q["status"])
        want = np.array([[unhex(v) for v in row] for row in q["path"]]).reshape(-1, P["dim"])
        path = o.path()
        assert path.shape == want.shape and np.array_equal(bits(path), bits(want)), k
        if q["status"] != "invalid_start":
            assert (len(o.start_connections()), len(o.goal_indices())) == (q["n_start"], q["n_goal"]), k
        if q["status"] == "solved":
            assert q["goal_node"] in o.goal_indices() and np.array_equal(bits(states[q["goal_node"]]), bits(path[-1])), k
        else:
            assert q["goal_node"] == -1
    assert "solved" in seen and "invalid_start" in seen


def test_batch_golden_so3_scene_is_recorded():
    """(the SO(3) scene has no C oracle: the device test checks it; here only its shape)"""
    with open(os.path.join(ROOT, "tests", "golden", "prm_batch_golden.json")) as f:
        rec = json.load(f)["fixture"]
    assert rec["space"] == "so3" and rec["n"] == 500 and len(rec["queries"]) == 32
    assert {q["status"] for q in rec["queries"]} == {"solved", "no_solution", "invalid_start"}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "prm_batch_golden.json")) < (1 << 20)
