"""CPU: the additions of DESIGN.md section 23 to the PRM ABI (oxhip_prm_grow_roadmap, oxhip_prm_grow_last_timing,
oxhip_prm_grow_config; prm_grow.hip).
(i)   header, capi.EXPORTS, the library and rust/oxmpl-hip/src/ffi.rs agree on the names and their arity; the ABI version is 2;
(ii)  oxhip_prm_grow_config is 32 bytes with the same field offsets in the header, the ctypes mirror and ffi.rs, and
      OXHIP_PRM_GROW_NEW_STREAM is 1 in all three;
(iii) null pointers and a wrong struct_size are OXHIP_ERR_BAD_ARG without a device;
(iv)  the Python, C++ and Rust mirrors carry the surface;
(v)   prm_grow.hip compiles for gfx950 and the compiler's per-kernel metadata shows no private segment and no spills;
(vi)  the expectation the GPU tests hold the device to (tests/prm_grow_helpers.py: expected_growth) treats dead milestones,
      ascending rows and symmetry as the issue states them, on hand-made inputs."""
import ctypes as C
import os
import re
import subprocess

import pytest

from oxmpl_amd import capi
from prm_grow_helpers import check_rows, expected_growth, make_near

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oxmpl_amd", "csrc")
NEW = {"oxhip_prm_grow_roadmap": 4, "oxhip_prm_grow_last_timing": 2}
LAYOUT = [("struct_size", 0, 4), ("n_more", 4, 4), ("max_samples", 8, 8), ("flags", 16, 4), ("pad", 20, 4), ("stream", 24, 8)]


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
    assert C.sizeof(capi.Config) == 232 and C.sizeof(capi.PrmConfig) == 200   # the two configuration structs are what they were


def test_grow_config_layout_and_flag_agree_everywhere(tmp_path):
    header = open(os.path.join(ROOT, "include", "oxmpl_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "oxmpl-hip", "src", "ffi.rs")).read()
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "oxmpl_hip.h"', 'int main(void) {',
            '  printf("size %zu\\n", sizeof(oxhip_prm_grow_config));', '  printf("flag %u\\n", OXHIP_PRM_GROW_NEW_STREAM);']
    for f, _, _ in LAYOUT:
        prog.append('  printf("%s %%zu %%zu\\n", offsetof(oxhip_prm_grow_config, %s), sizeof(((oxhip_prm_grow_config*)0)->%s));' % (f, f, f))
    prog.append('  return 0; }')
    src, exe = tmp_path / "grow_layout.c", tmp_path / "grow_layout"
    src.write_text("\n".join(prog))
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    assert out[0] == "size 32" and out[1] == "flag 1"
    assert [(l.split()[0], int(l.split()[1]), int(l.split()[2])) for l in out[2:] if l] == LAYOUT
    assert C.sizeof(capi.PrmGrowConfig) == 32
    assert [(n, getattr(capi.PrmGrowConfig, n).offset, getattr(capi.PrmGrowConfig, n).size) for n, _ in capi.PrmGrowConfig._fields_] == LAYOUT
    assert capi.PRM_GROW_NEW_STREAM == 1
    body = re.search(r"pub const OXHIP_PRM_GROW_CONFIG_LAYOUT: &\[\(&str, usize, usize\)\] = &\[(.*?)\];", ffi, re.S).group(1)
    assert [(m.group(1), int(m.group(2)), int(m.group(3))) for m in re.finditer(r'\("(\w+)",\s*(\d+),\s*(\d+)\)', body)] == LAYOUT
    assert re.search(r"pub const OXHIP_PRM_GROW_CONFIG_SIZE: usize = 32;", ffi)
    assert re.search(r"pub const OXHIP_PRM_GROW_NEW_STREAM: u32 = 1;", ffi)
    assert re.search(r"#define\s+OXHIP_PRM_GROW_NEW_STREAM\s+1u?\b", header)
    fields = re.search(r"pub struct OxhipPrmGrowConfig \{(.*?)\n\}", ffi, re.S).group(1)
    assert re.findall(r"pub (\w+): (\w+),", fields) == [("struct_size", "u32"), ("n_more", "u32"), ("max_samples", "u64"), ("flags", "u32"),
                                                       ("pad", "u32"), ("stream", "u64")]


def test_null_pointers_and_struct_size_are_bad_arg_without_a_device(L):
    g = capi.PrmGrowConfig()
    g.struct_size, g.n_more = C.sizeof(capi.PrmGrowConfig), 4
    added, drawn, d = C.c_uint32(7), C.c_uint64(7), (C.c_double * 6)()
    fake = C.c_void_p(1)   # never dereferenced: every refusal below precedes the first look at the handle
    assert L.oxhip_prm_grow_roadmap(None, C.byref(g), C.byref(added), C.byref(drawn)) == capi.ERR_BAD_ARG
    assert b"null" in L.oxhip_last_error_string()
    assert L.oxhip_prm_grow_roadmap(fake, None, C.byref(added), C.byref(drawn)) == capi.ERR_BAD_ARG
    assert L.oxhip_prm_grow_roadmap(fake, C.byref(g), None, C.byref(drawn)) == capi.ERR_BAD_ARG
    assert L.oxhip_prm_grow_roadmap(fake, C.byref(g), C.byref(added), None) == capi.ERR_BAD_ARG
    assert b"null" in L.oxhip_last_error_string()
    for size in (0, 24, 31, 33, 200):
        g.struct_size = size
        assert L.oxhip_prm_grow_roadmap(fake, C.byref(g), C.byref(added), C.byref(drawn)) == capi.ERR_BAD_ARG
        assert b"struct_size" in L.oxhip_last_error_string()
    g.struct_size, g.n_more = C.sizeof(capi.PrmGrowConfig), 0
    assert L.oxhip_prm_grow_roadmap(fake, C.byref(g), C.byref(added), C.byref(drawn)) == capi.ERR_BAD_ARG
    assert b"n_more" in L.oxhip_last_error_string()
    g.n_more, g.flags = 4, 2
    assert L.oxhip_prm_grow_roadmap(fake, C.byref(g), C.byref(added), C.byref(drawn)) == capi.ERR_BAD_ARG
    assert b"OXHIP_PRM_GROW_NEW_STREAM" in L.oxhip_last_error_string()
    assert L.oxhip_prm_grow_last_timing(None, d) == capi.ERR_BAD_ARG


def test_mirrors_have_the_surface():
    from oxmpl_amd.geometric import PRM
    assert callable(capi.PRMRoadmap.grow) and callable(capi.PRMRoadmap.grow_timing) and callable(PRM.grow_roadmap)
    hpp = open(os.path.join(ROOT, "include", "oxmpl", "oxmpl.hpp")).read()
    rs = open(os.path.join(ROOT, "rust", "oxmpl-hip", "src", "lib.rs")).read()
    assert re.search(r"\bgrow_roadmap\(", hpp) and "oxhip_prm_grow_roadmap" in hpp and "OXHIP_PRM_GROW_NEW_STREAM" in hpp
    assert "pub fn grow_roadmap(" in rs and "ffi::oxhip_prm_grow_roadmap" in rs and "ffi::OXHIP_PRM_GROW_NEW_STREAM" in rs
    from oxmpl_amd.base import ProblemDefinition
    with pytest.raises(Exception) as e:   # no setup(): the reference's message, before any library call
        PRM(1.0, 1.0, ProblemDefinition(None, None, None)).grow_roadmap(4)
    assert "setup() was not called" in str(e.value)


def _kernel_metadata(asm):
    meta = {}
    for block in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|"
                                                        r"group_segment_fixed_size|max_flat_workgroup_size):\s+(\d+)", block)}
    return meta


def test_prm_grow_kernels_resource_shape(tmp_path):
    """Every kernel of prm_grow.hip: private segment 0 (no scratch), both spill counts 0; and, as the file says of itself, no LDS
    and 256-thread workgroups."""
    out = str(tmp_path / "prm_grow.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                           "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "prm_grow.hip")], stderr=subprocess.DEVNULL)
    meta = _kernel_metadata(open(out).read())
    assert len(meta) == 2 and sum("prm_grow_keys_kernel" in k for k in meta) == 1 and sum("prm_grow_filter_kernel" in k for k in meta) == 1, sorted(meta)
    misses = [(name, m) for name, m in meta.items()
              if not (m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0
                      and m["group_segment_fixed_size"] == 0 and m["max_flat_workgroup_size"] == 256)]
    assert not misses, misses


# ---------------------------------------------------------------------------------------------------------------- the expectation
def _table(pairs):
    return lambda j, i: (j, i) in pairs


def test_expected_growth_skips_dead_milestones_and_keeps_old_rows():
    # 4 old milestones on a path 0 - 1 - 2 - 3; milestone 1 is dead and keeps its (stale) row; every pair is near, every motion valid
    old = [[1], [0, 2], [1, 3], [2]]
    rows = expected_growth(old, 6, [True, False, True, True], lambda j, i: True, lambda pairs: [True] * len(pairs))
    assert rows[:4] == [[1, 4, 5], [0, 2], [1, 3, 4, 5], [2, 4, 5]]      # the dead row gets nothing, the old parts are untouched
    assert rows[4] == [0, 2, 3, 5] and rows[5] == [0, 2, 3, 4]          # a milestone of this call is live for the later ones
    check_rows(rows)
    assert all(1 not in r for r in rows[4:])


def test_expected_growth_asks_near_and_motion_in_construction_s_direction():
    asked = []

    def motion(pairs):
        asked.extend(pairs)
        return [(j, i) != (4, 0) for j, i in pairs]                      # one motion between two live ends is invalid
    near = _table({(3, 0), (3, 1), (4, 0), (4, 3), (5, 2)})              # (5, 2): 2 is dead; (3, 2) is not near
    rows = expected_growth([[], [], []], 6, [True, True, False], near, motion)
    assert asked == [(3, 0), (3, 1), (4, 0), (4, 3)]                     # from the new milestone to the earlier one; never a dead end
    assert rows == [[3], [3], [], [0, 1, 4], [3], []]
    check_rows(rows)


def test_expected_growth_without_dead_milestones_is_construction_s_rule():
    # every old milestone live: the rows equal what the loop of prm.rs:117-147 builds from scratch over the same tables
    near = _table({(j, i) for j in range(9) for i in range(j) if (j * 7 + i * 3) % 4 != 0})
    bad = {(5, 1), (7, 2), (8, 6)}
    from_scratch = expected_growth([], 9, [], near, lambda pairs: [p not in bad for p in pairs])
    first = expected_growth([], 4, [], near, lambda pairs: [p not in bad for p in pairs])
    grown = expected_growth(first, 9, [True] * 4, near, lambda pairs: [p not in bad for p in pairs])
    assert grown == from_scratch and grown[5].count(1) == 0 and 8 not in grown[6]
    check_rows(grown)
    with pytest.raises(AssertionError):
        check_rows([[1], []])                                            # the checker itself sees an asymmetric row


def test_make_near_is_the_strict_radius_test_with_the_new_milestone_first():
    calls = []

    def dist(a, b):
        calls.append((tuple(a), tuple(b)))
        return abs(a[0] - b[0])
    states = [[0.0], [1.0], [5.0], [2.0]]
    near = make_near(states, 2, 1.0, dist)
    assert [near(3, 0), near(3, 1), near(3, 2), near(2, 0)] == [False, False, False, False]   # 3 - 1 is exactly the radius: not near
    near = make_near(states, 2, 1.0000001, dist)
    assert near(3, 1) and not near(3, 0)
    assert ((2.0,), (1.0,)) in calls and ((1.0,), (2.0,)) not in calls
