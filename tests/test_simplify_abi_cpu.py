"""CPU: the path entry points of the RRT batch (oxhip_rrt_batch_extract_paths .. oxhip_rrt_batch_paths_last_timing,
path_simplify.hip and shortcut_core.hip).
(i)   header, capi.EXPORTS, the library and rust/oxmpl-hip/src/ffi.rs agree on the names and their arity; the ABI version and
      both configuration structs are what they were;
(ii)  null handles and null pointers are OXHIP_ERR_BAD_ARG;
(iii) without a device the Python mirror reaches ERR_NO_DEVICE at setup, not a crash, and simplify_solution before setup() is
      the reference's "uninitialised" message;
(iv)  path_simplify.hip and shortcut_core.hip compile for gfx950 with exactly their instantiations, without scratch, VGPR spills or
      flat / scratch memory instructions, and every shortcut kernel is a symbol of one object of the library alone."""
import ctypes as C
import os
import re
import subprocess

import pytest

from oxmpl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oxmpl_amd", "csrc")
NEW = {"oxhip_rrt_batch_extract_paths": 1, "oxhip_rrt_batch_get_paths": 5, "oxhip_rrt_batch_simplify_paths": 3,
       "oxhip_rrt_batch_get_simplified_paths": 6, "oxhip_rrt_batch_get_simplify_results": 4,
       "oxhip_rrt_batch_path_valid_matrix": 6, "oxhip_rrt_batch_paths_last_timing": 5}


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
    for m in ("extract_paths", "paths", "simplify_paths", "simplified_paths"):
        assert callable(getattr(capi.RRTBatch, m))


def test_null_handles_and_pointers_are_bad_arg(L):
    d, u8, u32, u64 = (C.c_double * 8)(), (C.c_uint8 * 4)(), (C.c_uint32 * 2)(), (C.c_uint64 * 3)()
    assert L.oxhip_rrt_batch_extract_paths(None) == capi.ERR_BAD_ARG
    assert L.oxhip_rrt_batch_get_paths(None, u64, d, 1, u64) == capi.ERR_BAD_ARG
    assert L.oxhip_rrt_batch_simplify_paths(None, 0, 0) == capi.ERR_BAD_ARG
    assert L.oxhip_rrt_batch_get_simplified_paths(None, u64, d, u32, 1, u64) == capi.ERR_BAD_ARG
    assert L.oxhip_rrt_batch_get_simplify_results(None, d, d, u64) == capi.ERR_BAD_ARG
    assert L.oxhip_rrt_batch_path_valid_matrix(None, 0, 0, u8, 4, u32) == capi.ERR_BAD_ARG
    assert L.oxhip_rrt_batch_paths_last_timing(None, d, d, d, u32) == capi.ERR_BAD_ARG
    assert b"null" in L.oxhip_last_error_string()


def test_python_mirror_without_a_device(L):
    from oxmpl_amd.base import ProblemDefinition, RealVectorState, RealVectorStateSpace, SphereBoxValidityChecker
    from oxmpl_amd.geometric import RRT, RRTConnect, RRTStar, _MESSAGES

    class Goal:
        def __init__(self, target, radius):
            self.target, self.radius = target, radius

    space = RealVectorStateSpace(2, [(0.0, 10.0), (0.0, 10.0)])
    pd = ProblemDefinition(space, RealVectorState([1.0, 5.0]), Goal(RealVectorState([9.0, 5.0]), 0.5))
    for planner in (RRT(0.5, 0.05, pd), RRTConnect(0.5, 0.05, pd), RRTStar(0.5, 0.05, 1.0, pd)):
        with pytest.raises(Exception) as ei:
            planner.simplify_solution()
        assert str(ei.value) == _MESSAGES[capi.ERR_PLANNER_UNINITIALISED]
    n = C.c_int32()
    if L.oxhip_device_count(C.byref(n)) == capi.OK:
        return                                  # (the rest is about a machine without a device)
    with pytest.raises(capi.OxhipError) as ei:  # no batch can exist without a device: the new entry points are never reached
        RRT(0.5, 0.05, pd).setup(SphereBoxValidityChecker(boxes=[([4.75, 2.0], [5.25, 8.0])]))
    assert ei.value.status == capi.ERR_NO_DEVICE
    with pytest.raises(capi.OxhipError) as ei:
        capi.RRTBatch(2, [(0.0, 10.0), (0.0, 10.0)], 0.5, 0.05, 4)
    assert ei.value.status == capi.ERR_NO_DEVICE


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
    asm = open(out).read()
    return asm, _kernels(asm)


def _instances(meta, kernel, suffix=""):
    """the D of every kernel<D, ...suffix> in the metadata ("n1" is -1)"""
    return sorted(re.search(kernel + r"ILi(n?\d+)E" + suffix + "E", k).group(1) for k in meta if re.search(kernel + r"ILin?\d+E" + suffix + "E", k))


def test_path_simplify_kernels_resource_shape(tmp_path, L):
    asm, meta = _compile(tmp_path, "path_simplify.hip")
    assert sorted(re.search(r"path_\w+_kernel", k).group(0) for k in meta) == ["path_len_kernel", "path_rows_kernel"]   # the chain walks alone
    core_asm, core = _compile(tmp_path, "shortcut_core.hip")
    # the pair matrix with m = 1 in R^2 .. R^8, SO(3) and SO(2), subdivided in R^1 .. R^8 and SO(3); the DP in all of them
    rn = [str(d) for d in range(2, 9)]
    assert _instances(core, "shortcut_pairs_kernel", "Lb0") == sorted(rn + ["0", "n1"])
    assert _instances(core, "shortcut_pairs_kernel", "Lb1") == sorted(rn + ["0", "1"])
    assert _instances(core, "shortcut_dp_kernel") == sorted(rn + ["0", "1", "n1"])
    assert len(core) == 9 + 9 + 10 and all("shortcut_pairs_kernel" in k or "shortcut_dp_kernel" in k for k in core)
    for text, kernels in ((asm, meta), (core_asm, core)):
        for name, m in kernels.items():
            assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
            assert m["max_flat_workgroup_size"] == (256 if "shortcut_pairs_kernel" in name else 64), (name, m)
            body = text.split("\n" + name + ":")[1].split("s_endpgm")[0]
            assert len(body) > 200, name
            assert "flat_load" not in body and "scratch_" not in body, name
    # one definition: every shortcut kernel is a symbol of exactly one of the library's objects
    srcs = re.search(r"^SRCS\s*:=(.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
    assert "shortcut_core.hip" in srcs and "path_simplify.hip" in srcs
    objects = {src: open(os.path.join(CSRC, src[:-4] + ".o"), "rb").read() for src in srcs}   # (the fixture built them)
    for name in core:
        assert [src for src, blob in objects.items() if name.encode() in blob] == ["shortcut_core.hip"], name
    for gone in (b"path_pairs_kernel", b"path_dp_kernel", b"dense_pairs_kernel", b"dense_dp_kernel"):
        assert not [src for src, blob in objects.items() if gone in blob], gone
