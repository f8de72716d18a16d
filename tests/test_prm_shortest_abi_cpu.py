"""CPU: the shortest-path additions to the PRM ABI (oxhip_prm_solve_batch_shortest, oxhip_prm_batch_get_costs, _get_labels and the
diagnostic _get_search_stats; prm_shortest.hip).
(i)   header, capi.EXPORTS, the library and rust/oxmpl-hip/src/ffi.rs agree on the names and their arity; the ABI version and both
      configuration structs are what they were;
(ii)  null handles and null pointers are OXHIP_ERR_BAD_ARG;
(iii) prm_shortest.hip compiles for gfx950 with no private segment, no spills and no flat / scratch memory instructions."""
import ctypes as C
import os
import re
import subprocess

import pytest

from oxmpl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oxmpl_amd", "csrc")
NEW = {"oxhip_prm_solve_batch_shortest": 9, "oxhip_prm_batch_get_costs": 2, "oxhip_prm_batch_get_labels": 6,
       "oxhip_prm_batch_get_search_stats": 4}


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
    for weights in (0, 1, 2, 3):
        assert L.oxhip_prm_solve_batch_shortest(None, 1, d, d, d, 0.0, 0, weights, i32) == capi.ERR_BAD_ARG
    assert L.oxhip_prm_solve_batch_shortest(None, 0, None, None, None, 0.0, 0, 0, None) == capi.ERR_BAD_ARG
    assert L.oxhip_prm_batch_get_costs(None, d) == capi.ERR_BAD_ARG
    assert L.oxhip_prm_batch_get_labels(None, 0, d, u32, u32, 2) == capi.ERR_BAD_ARG
    assert L.oxhip_prm_batch_get_search_stats(None, u32, u64, d) == capi.ERR_BAD_ARG
    assert b"null" in L.oxhip_last_error_string()


def test_python_mirror_has_the_surface():
    import inspect
    from oxmpl_amd.geometric import PRM
    for name in ("solve_batch_shortest", "batch_costs", "batch_labels", "batch_search_stats"):
        assert callable(getattr(capi.PRMRoadmap, name))
    assert inspect.signature(capi.PRMRoadmap.solve_batch_shortest).parameters["weights"].default == 0
    assert inspect.signature(PRM.solve_batch).parameters["shortest"].default is False


def _kernels(asm):
    """name -> (metadata, instructions of the body)"""
    meta = {}
    for block in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(r"\.(vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", block)}
    return {name: (m, asm.split("\n" + name + ":")[1].split(".Lfunc_end")[0]) for name, m in meta.items()}


def test_prm_shortest_kernels_resource_shape(tmp_path):
    out = str(tmp_path / "prm_shortest.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                           "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "prm_shortest.hip")], stderr=subprocess.DEVNULL)
    kernels = _kernels(open(out).read())
    assert len(kernels) >= 4 and all("prm_shortest_" in k for k in kernels)
    for name, (m, body) in kernels.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert not re.search(r"\b(flat|scratch)_(load|store|atomic)", body), name
        assert len(body) > 200, name
