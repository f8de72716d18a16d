"""CPU: the additions of DESIGN.md section 21 to the RRT batch ABI (oxhip_rrt_batch_revalidate_trees,
oxhip_rrt_batch_get_revalidate_map, oxhip_rrt_batch_revalidate_last_timing; rrt_revalidate.hip).
(i)   header, capi.EXPORTS, the library and rust/oxmpl-hip/src/ffi.rs agree on the names and their arity; the ABI version and both
      configuration structs are what they were;
(ii)  null handles and null pointers are OXHIP_ERR_BAD_ARG, not crashes;
(iii) the Python, C++ and Rust mirrors carry the surface;
(iv)  rrt_revalidate.hip compiles for gfx950 and the compiler's per-kernel metadata shows no private segment, no spills and
      fewer than 128 VGPRs for every kernel (only those directives are read);
(v)   the numpy half of the GPU tests' oracle (tests/rrt_revalidate_helpers.py) reproduces tests/golden/rrt_revalidate.json, which
      a pure-Python generator wrote from the existing restatements of check_motion."""
import ctypes as C
import json
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

from oxmpl_amd import capi

import rrt_revalidate_helpers as rh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oxmpl_amd", "csrc")
NEW = {"oxhip_rrt_batch_revalidate_trees": 3, "oxhip_rrt_batch_get_revalidate_map": 6, "oxhip_rrt_batch_revalidate_last_timing": 2}


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
    d, u8, u32, i32 = (C.c_double * 4)(), (C.c_uint8 * 4)(), (C.c_uint32 * 4)(), (C.c_int32 * 4)()
    assert L.oxhip_rrt_batch_revalidate_trees(None, u32, u8) == capi.ERR_BAD_ARG
    assert b"null" in L.oxhip_last_error_string()
    assert L.oxhip_rrt_batch_revalidate_trees(None, None, None) == capi.ERR_BAD_ARG
    assert L.oxhip_rrt_batch_get_revalidate_map(None, 0, i32, u8, 4, u32) == capi.ERR_BAD_ARG
    assert L.oxhip_rrt_batch_get_revalidate_map(None, 0, None, None, 0, None) == capi.ERR_BAD_ARG
    assert L.oxhip_rrt_batch_revalidate_last_timing(None, d) == capi.ERR_BAD_ARG
    assert L.oxhip_rrt_batch_revalidate_last_timing(None, None) == capi.ERR_BAD_ARG
    assert b"null" in L.oxhip_last_error_string()


def test_mirrors_have_the_surface():
    from oxmpl_amd.geometric import RRT, RRTConnect, RRTStar
    for name in ("revalidate_trees", "revalidate_map", "revalidate_last_timing"):
        assert callable(getattr(capi.RRTBatch, name))
    assert callable(RRT.revalidate)
    for cls, args in ((RRTConnect, (0.5, 0.05)), (RRTStar, (0.5, 0.05, 1.0))):   # refused before anything touches a device
        from oxmpl_amd.base import ProblemDefinition
        with pytest.raises(TypeError):
            cls(*args, ProblemDefinition(None, None, None)).revalidate()
    hpp = open(os.path.join(ROOT, "include", "oxmpl", "oxmpl.hpp")).read()
    rs = open(os.path.join(ROOT, "rust", "oxmpl-hip", "src", "lib.rs")).read()
    assert re.search(r"\brevalidate\(", hpp) and "oxhip_rrt_batch_revalidate_trees" in hpp
    assert "ffi::oxhip_rrt_batch_revalidate_trees" in rs
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_rrt_revalidate_rvss.cpp"))


def _kernel_metadata(asm):
    meta = {}
    for block in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|"
                                                        r"max_flat_workgroup_size):\s+(\d+)", block)}
    return meta


def test_rrt_revalidate_kernels_resource_shape(tmp_path):
    """What the issue set: private segment 0, both spill counts 0, fewer than 128 VGPRs, for every new kernel (the widest,
    rrt_reval_edge_kernel<8>: 116 VGPRs).  SO(3) edges are checked by the kernel behind oxhip_rrt_batch_check_motion
    (so3_check_motion_kernel of rrt_so3.hip, not a new kernel) on staged rows: a new kernel around either SO(3) motion function
    kept exec masks in four spilled SGPRs."""
    out = str(tmp_path / "rrt_revalidate.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                           "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "rrt_revalidate.hip")], stderr=subprocess.DEVNULL)
    own = {k: m for k, m in _kernel_metadata(open(out).read()).items() if "rrt_reval_" in k}
    for family, count in (("rrt_reval_edge_kernel", 9), ("rrt_reval_stage_kernel", 1), ("rrt_reval_unstage_kernel", 1),
                          ("rrt_reval_survive_kernel", 1), ("rrt_reval_scan_kernel", 1),
                          ("rrt_reval_compact_kernel", 10), ("rrt_reval_skip_kernel", 10)):   # R^1 .. R^8, DIM = -1: SO(2) (and DIM = 0: SO(3))
        assert sum(1 for k in own if family in k) == count, (family, sorted(own))
    assert len(own) == 33
    misses = [(name, m) for name, m in own.items()
              if not (m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0
                      and m["vgpr_count"] < 128 and m["max_flat_workgroup_size"] == 256)]
    assert not misses, misses   # (every kernel is judged: the message lists exactly the ones that miss)


# ------------------------------------------------------------------------------------------------ (v) the oracle's own half
def _crc(arr, dtype):
    return "%08x" % (zlib.crc32(np.ascontiguousarray(arr, dtype=dtype).tobytes()) & 0xFFFFFFFF)


@pytest.fixture(scope="module")
def reval_golden():
    with open(os.path.join(ROOT, "tests", "golden", "rrt_revalidate.json")) as f:
        return json.load(f)


def test_golden_covers_the_planted_scenes(reval_golden):
    scenes = rh.planted_scenes()
    assert set(scenes) == {k for k in reval_golden if k not in ("_generator", "fraction")}
    for name, (_, partial) in scenes.items():
        g = reval_golden[name]
        n = g["trees"][2]["n"]
        assert g["partial"] == partial and g["trees"][0]["n_removed"] == 0 and g["trees"][1]["n_removed"] == n - 1
        if partial:
            assert 0 < g["trees"][2]["n_removed"] < n - 1, name
    # the cases the issue names are there and say what they should
    assert reval_golden["r2_chain2049_cut1"]["trees"][2]["n_removed"] == 2048
    assert reval_golden["r2_chain2049_cut1000"]["trees"][2]["failed_edges"] == [1000]
    assert reval_golden["r2_chain2049_cut2048"]["trees"][2]["failed_edges"] == [2048]
    t = reval_golden["r3_twins"]["trees"][2]
    assert t["new_index"][11] == -1 and t["new_index"][40] >= 0 and t["skip"][t["new_index"][40]] == 0    # the lower twin died
    assert t["new_index"][41] == -1 and t["skip"][t["new_index"][10]] == 0                               # the higher twin died
    assert t["skip"][t["new_index"][50]] == 1 and t["new_index"][13] == t["new_index"][51] == -1          # neither / both
    g = reval_golden["r3_goal_lost"]["trees"][2]
    assert g["goal_before"] >= 1 and g["goal_after"] == -1
    g = reval_golden["r3_goal_kept"]["trees"][2]
    assert 1 <= g["goal_after"] < g["goal_before"]
    g = reval_golden["r3_goal_root"]["trees"][2]
    assert g["in_goal"] == [0] and g["goal_before"] == g["goal_after"] == -1


@pytest.mark.parametrize("name", sorted(rh.planted_scenes()))
def test_helper_reproduces_the_golden_file(name, reval_golden):
    scene = rh.planted_scenes()[name][0]()
    for (states, parents), g in zip(scene["trees"], reval_golden[name]["trees"]):
        n = len(parents)
        assert n == g["n"] and _crc(states, np.float64) == g["states_crc"]   # the same planted tree
        edge_ok = np.ones(n, dtype=bool)
        edge_ok[g["failed_edges"]] = False
        sat = np.zeros(n, dtype=bool)
        sat[g["in_goal"]] = True
        exp = rh.expected(states, parents, edge_ok, sat)
        assert exp["n_removed"] == g["n_removed"] and exp["goal_node"] == g["goal_after"] and rh.goal_node(sat) == g["goal_before"]
        assert _crc(exp["new_index"], np.int32) == g["new_index_crc"] and _crc(exp["parents"], np.int32) == g["parents_crc"]
        assert _crc(exp["skip"], np.uint8) == g["skip_crc"] and [int(i) for i in np.flatnonzero(exp["skip"])] == g["skip_set"]
        if "new_index" in g:
            assert list(exp["new_index"]) == g["new_index"] and list(exp["parents"]) == g["parents"] and list(exp["skip"]) == g["skip"]
