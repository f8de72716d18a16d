"""CPU: the additions of DESIGN.md section 20 to the PRM ABI (oxhip_prm_set_roadmap, oxhip_prm_revalidate,
oxhip_prm_revalidate_last_timing; prm_revalidate.hip).
(i)   header, capi.EXPORTS, the library and rust/oxmpl-hip/src/ffi.rs agree on the names and their arity; the ABI version and both
      configuration structs are what they were;
(ii)  null handles and null pointers are OXHIP_ERR_BAD_ARG, not crashes;
(iii) the Python, C++ and Rust mirrors carry the surface;
(iv)  prm_revalidate.hip compiles for gfx950 and the compiler's per-kernel metadata shows no private segment, no spills and
      fewer than 128 VGPRs for every kernel (only those directives are read)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from oxmpl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oxmpl_amd", "csrc")
NEW = {"oxhip_prm_set_roadmap": 5, "oxhip_prm_revalidate": 4, "oxhip_prm_revalidate_last_timing": 2}


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
    d, u8, u32, u64 = (C.c_double * 8)(), (C.c_uint8 * 4)(), (C.c_uint32 * 4)(), (C.c_uint64 * 4)()
    assert L.oxhip_prm_set_roadmap(None, d, 2, u64, u32) == capi.ERR_BAD_ARG
    assert b"null" in L.oxhip_last_error_string()
    assert L.oxhip_prm_set_roadmap(None, None, 0, None, None) == capi.ERR_BAD_ARG
    assert L.oxhip_prm_revalidate(None, u8, u32, u64) == capi.ERR_BAD_ARG
    assert L.oxhip_prm_revalidate(None, None, None, None) == capi.ERR_BAD_ARG
    assert L.oxhip_prm_revalidate_last_timing(None, d) == capi.ERR_BAD_ARG
    assert b"null" in L.oxhip_last_error_string()


def test_mirrors_have_the_surface():
    from oxmpl_amd.geometric import PRM
    for name in ("set_roadmap", "revalidate", "revalidate_last_timing"):
        assert callable(getattr(capi.PRMRoadmap, name))
    for name in ("set_roadmap", "revalidate", "save_roadmap", "load_roadmap"):
        assert callable(getattr(PRM, name))
    hpp = open(os.path.join(ROOT, "include", "oxmpl", "oxmpl.hpp")).read()
    rs = open(os.path.join(ROOT, "rust", "oxmpl-hip", "src", "lib.rs")).read()
    for name in ("set_roadmap", "revalidate"):
        assert re.search(r"\b%s\(" % name, hpp) and "oxhip_prm_" + name in hpp
        assert "pub fn %s(" % name in rs and "ffi::oxhip_prm_" + name in rs


def _kernel_metadata(asm):
    meta = {}
    for block in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|"
                                                        r"group_segment_fixed_size|max_flat_workgroup_size):\s+(\d+)", block)}
    return meta


def test_prm_revalidate_kernels_resource_shape(tmp_path):
    """What the issue set: private segment 0, both spill counts 0, fewer than 128 VGPRs, for every new kernel (the widest,
    prm_reval_check_kernel<8>: 104 SGPRs, 110 VGPRs).  SO(3) motions are checked by construction's own prm_so3_edge_kernel
    (prm_so3.hip, not a new kernel; tests/test_prm_so3_abi_cpu.py reads its shape): a new kernel around so3_motion_valid_seq kept
    an exec mask of that function in two spilled SGPRs whatever was moved out of its way."""
    out = str(tmp_path / "prm_revalidate.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                           "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "prm_revalidate.hip")], stderr=subprocess.DEVNULL)
    meta = _kernel_metadata(open(out).read())
    own = {k: m for k, m in meta.items() if "prm_plant_" in k or "prm_reval_" in k}   # (the rest are the scan library's)
    for family, count in (("prm_plant_offsets_kernel", 1), ("prm_plant_entries_kernel", 1),
                          ("prm_reval_valid_kernel", 9), ("prm_reval_valid_kernelILi0E", 1),   # R^1 .. R^8 and DIM = 0: SO(3)
                          ("prm_reval_emit_kernel", 1), ("prm_reval_check_kernel", 8),
                          ("prm_reval_keys_kernel", 1), ("prm_reval_mirror_kernel", 1), ("prm_reval_compact_kernel", 1)):
        assert sum(1 for k in own if family in k) == count, (family, sorted(own))
    assert len(own) == 23
    misses = [(name, m) for name, m in own.items()
              if not (m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0
                      and m["vgpr_count"] < 128
                      and m["group_segment_fixed_size"] == 0 and m["max_flat_workgroup_size"] == 256)]   # no LDS; 256-thread workgroups
    assert not misses, misses   # (every kernel is judged: the message lists exactly the ones that miss)
