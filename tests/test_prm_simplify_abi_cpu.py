"""CPU: the PRM handle's checker and shortcut entry points (oxhip_prm_is_valid .. oxhip_prm_batch_simplify_last_timing,
prm_path_simplify.hip and shortcut_core.hip).
(i)   header, capi.EXPORTS, the library and rust/oxmpl-hip/src/ffi.rs agree on the seven names and their arity; the ABI version
      and both configuration structs are what they were;
(ii)  null handles and null pointers are OXHIP_ERR_BAD_ARG;
(iii) the Python mirror's simplify calls before setup() carry the reference's "uninitialised" message;
(iv)  prm_path_simplify.hip compiles for gfx950 with exactly the instantiations D = 1 .. 8 and 0 of its templated kernel, and
      shortcut_core.hip with the subdivided pair matrix in the same spaces, without scratch or VGPR spills (from the code objects'
      metadata alone)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from oxmpl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oxmpl_amd", "csrc")
NEW = {"oxhip_prm_is_valid": 4, "oxhip_prm_check_motion": 5, "oxhip_prm_batch_simplify_paths": 4,
       "oxhip_prm_batch_get_simplified_paths": 6, "oxhip_prm_batch_get_simplify_results": 4,
       "oxhip_prm_batch_path_valid_matrix": 7, "oxhip_prm_batch_simplify_last_timing": 3}


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
    for m in ("is_valid", "check_motion", "simplify_batch_paths", "simplified_batch_paths", "simplify_results",
              "batch_path_valid_matrix", "simplify_timing"):
        assert callable(getattr(capi.PRMRoadmap, m))
    lib_rs = open(os.path.join(ROOT, "rust", "oxmpl-hip", "src", "lib.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "oxmpl", "oxmpl.hpp")).read()
    assert "pub fn simplify_batch" in lib_rs and "oxhip_prm_batch_simplify_paths" in lib_rs
    for call in ("oxhip_prm_is_valid", "oxhip_prm_check_motion", "oxhip_prm_batch_simplify_paths"):
        assert call in hpp


def test_null_handles_and_pointers_are_bad_arg(L):
    d, u8, u32, u64 = (C.c_double * 8)(), (C.c_uint8 * 4)(), (C.c_uint32 * 2)(), (C.c_uint64 * 3)()
    assert L.oxhip_prm_is_valid(None, d, 1, u8) == capi.ERR_BAD_ARG
    assert L.oxhip_prm_check_motion(None, d, d, 1, u8) == capi.ERR_BAD_ARG
    assert L.oxhip_prm_batch_simplify_paths(None, 1, 0, 0) == capi.ERR_BAD_ARG
    assert L.oxhip_prm_batch_get_simplified_paths(None, u64, d, u32, 1, u64) == capi.ERR_BAD_ARG
    assert L.oxhip_prm_batch_get_simplify_results(None, d, d, u64) == capi.ERR_BAD_ARG
    assert L.oxhip_prm_batch_path_valid_matrix(None, 0, 1, 0, u8, 4, u32) == capi.ERR_BAD_ARG
    assert L.oxhip_prm_batch_simplify_last_timing(None, d, u32) == capi.ERR_BAD_ARG
    assert b"null" in L.oxhip_last_error_string()


def test_python_mirror_before_setup():
    from oxmpl_amd.base import ProblemDefinition, RealVectorState, RealVectorStateSpace
    from oxmpl_amd.geometric import PRM, _MESSAGES

    class Goal:
        def __init__(self, target, radius):
            self.target, self.radius = target, radius

    space = RealVectorStateSpace(2, [(0.0, 10.0), (0.0, 10.0)])
    pd = ProblemDefinition(space, RealVectorState([1.0, 5.0]), Goal(RealVectorState([9.0, 5.0]), 0.5))
    for call in (lambda p: p.simplify_batch(), lambda p: p.simplify_solution(subdivide=4)):
        with pytest.raises(Exception) as ei:
            call(PRM(1.0, 0.5, pd))
        assert str(ei.value) == _MESSAGES[capi.ERR_PLANNER_UNINITIALISED]


def _kernels(asm):
    meta = {}
    for block in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|private_segment_fixed_size|"
                                                        r"group_segment_fixed_size|max_flat_workgroup_size):\s+(\d+)", block)}
    return meta


def _compile(tmp_path, src):
    out = str(tmp_path / (src[:-4] + ".s"))
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                           "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, src)], stderr=subprocess.DEVNULL)
    return _kernels(open(out).read())


def test_prm_path_simplify_kernels_resource_shape(tmp_path):
    meta = _compile(tmp_path, "prm_path_simplify.hip")
    got = sorted(re.search(r"dense_rows_kernelILi(n?\d+)E", k).group(1) for k in meta if "dense_rows_kernel" in k)
    assert got == sorted(str(d) for d in range(0, 9)), got                    # D = 1 .. 8 and 0 (SO(3)); no SO(2) ("n1")
    assert sum("dense_gather_kernel" in k for k in meta) == 1 and len(meta) == 9 + 1
    # the pair matrix and the DP over the dense rows are shortcut_core.hip's: subdivided in the same spaces, and the DP in SO(2) too
    core = _compile(tmp_path, "shortcut_core.hip")
    for kernel, suffix, dims in (("shortcut_pairs_kernel", "Lb1", range(0, 9)), ("shortcut_dp_kernel", "", range(-1, 9))):
        got = sorted(re.search(kernel + r"ILi(n?\d+)E" + suffix + "E", k).group(1) for k in core if re.search(kernel + r"ILin?\d+E" + suffix + "E", k))
        assert got == sorted(str(d).replace("-", "n") for d in dims), (kernel, got)
    for name, m in list(meta.items()) + list(core.items()):
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert m["max_flat_workgroup_size"] == (64 if "shortcut_dp_kernel" in name or "dense_gather_kernel" in name else 256), (name, m)
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    for src in ("prm_path_simplify.hip", "shortcut_core.hip"):
        assert re.search(r"^SRCS\s*:=.*\b" + re.escape(src) + r"\b", makefile, re.M), src
