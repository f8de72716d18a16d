"""CPU: the additions of DESIGN.md section 24 to the PRM ABI (oxhip_prm_components, oxhip_prm_components_last_timing,
oxhip_prm_prune, oxhip_prm_prune_last_timing, oxhip_prm_prune_config; prm_components.hip).
(i)   header, capi.EXPORTS, the library and rust/oxmpl-hip/src/ffi.rs agree on the four names and their arity; the ABI version is 2;
(ii)  oxhip_prm_prune_config is 16 bytes with the same field offsets in the header (a compiled C probe), the ctypes mirror and
      ffi.rs, and the four OXHIP_PRM_PRUNE_* flags have the same values in all three;
(iii) every argument refusal happens without a device and before the handle is dereferenced;
(iv)  the Python, C++ and Rust mirrors carry the surface;
(v)   prm_components.hip compiles for gfx950 and the compiler's per-kernel metadata shows 256-thread workgroups, no private
      segment, no spills and no LDS; the kernel files other tests count by name hold none of the new kernels."""
import ctypes as C
import os
import re
import subprocess

import pytest

from oxmpl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oxmpl_amd", "csrc")
NEW = {"oxhip_prm_components": 7, "oxhip_prm_components_last_timing": 3, "oxhip_prm_prune": 6, "oxhip_prm_prune_last_timing": 2}
LAYOUT = [("struct_size", 0, 4), ("flags", 4, 4), ("min_size", 8, 4), ("pad", 12, 4)]
FLAGS = [("INVALID", 1), ("MASK", 2), ("MIN_SIZE", 4), ("LARGEST", 8)]


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
    assert C.sizeof(capi.Config) == 232 and C.sizeof(capi.PrmConfig) == 200 and C.sizeof(capi.PrmGrowConfig) == 32   # as they were


def test_prune_config_layout_and_flags_agree_everywhere(tmp_path):
    header = open(os.path.join(ROOT, "include", "oxmpl_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "oxmpl-hip", "src", "ffi.rs")).read()
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "oxmpl_hip.h"', 'int main(void) {',
            '  printf("size %zu\\n", sizeof(oxhip_prm_prune_config));',
            '  printf("flags %u %u %u %u\\n", OXHIP_PRM_PRUNE_INVALID, OXHIP_PRM_PRUNE_MASK, OXHIP_PRM_PRUNE_MIN_SIZE, OXHIP_PRM_PRUNE_LARGEST);']
    for f, _, _ in LAYOUT:
        prog.append('  printf("%s %%zu %%zu\\n", offsetof(oxhip_prm_prune_config, %s), sizeof(((oxhip_prm_prune_config*)0)->%s));' % (f, f, f))
    prog.append('  return 0; }')
    src, exe = tmp_path / "prune_layout.c", tmp_path / "prune_layout"
    src.write_text("\n".join(prog))
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    assert out[0] == "size 16" and out[1] == "flags 1 2 4 8"
    assert [(l.split()[0], int(l.split()[1]), int(l.split()[2])) for l in out[2:] if l] == LAYOUT
    assert C.sizeof(capi.PrmPruneConfig) == 16
    assert [(n, getattr(capi.PrmPruneConfig, n).offset, getattr(capi.PrmPruneConfig, n).size) for n, _ in capi.PrmPruneConfig._fields_] == LAYOUT
    body = re.search(r"pub const OXHIP_PRM_PRUNE_CONFIG_LAYOUT: &\[\(&str, usize, usize\)\] = &\[(.*?)\];", ffi, re.S).group(1)
    assert [(m.group(1), int(m.group(2)), int(m.group(3))) for m in re.finditer(r'\("(\w+)",\s*(\d+),\s*(\d+)\)', body)] == LAYOUT
    assert re.search(r"pub const OXHIP_PRM_PRUNE_CONFIG_SIZE: usize = 16;", ffi)
    fields = re.search(r"pub struct OxhipPrmPruneConfig \{(.*?)\n\}", ffi, re.S).group(1)
    assert re.findall(r"pub (\w+): (\w+),", fields) == [("struct_size", "u32"), ("flags", "u32"), ("min_size", "u32"), ("pad", "u32")]
    for name, value in FLAGS:
        assert getattr(capi, "PRM_PRUNE_" + name) == value
        assert re.search(r"pub const OXHIP_PRM_PRUNE_%s: u32 = %d;" % (name, value), ffi)
        assert re.search(r"#define\s+OXHIP_PRM_PRUNE_%s\s+%du\b" % (name, value), header)


def _config(flags, min_size=0, pad=0, struct_size=16):
    c = capi.PrmPruneConfig()
    c.struct_size, c.flags, c.min_size, c.pad = struct_size, flags, min_size, pad
    return c


def test_argument_refusals_need_no_device_and_no_handle(L):
    fake = C.c_void_p(1)   # never dereferenced: every refusal below precedes the first look at the handle
    idx, kept, removed = (C.c_int32 * 4)(), C.c_uint32(7), C.c_uint64(7)
    mask = (C.c_uint8 * 4)(1, 1, 1, 1)

    def prune(h, c, keep=None):
        return L.oxhip_prm_prune(h, None if c is None else C.byref(c), keep, idx, C.byref(kept), C.byref(removed))

    def refused(h, c, keep, word):
        assert prune(h, c, keep) == capi.ERR_BAD_ARG
        assert word in L.oxhip_last_error_string(), (word, L.oxhip_last_error_string())
    refused(None, _config(capi.PRM_PRUNE_INVALID), None, b"null")
    refused(fake, None, None, b"null")
    for size in (0, 8, 15, 17, 32):
        refused(fake, _config(capi.PRM_PRUNE_INVALID, struct_size=size), None, b"struct_size")
    refused(fake, _config(0), None, b"flags")
    for unknown in (16, 1 | 16, 0x80000000, 0xFFFFFFFF):
        refused(fake, _config(unknown), None, b"unknown flag")
    refused(fake, _config(capi.PRM_PRUNE_INVALID, pad=1), None, b"pad")
    refused(fake, _config(capi.PRM_PRUNE_MASK), None, b"keep")
    refused(fake, _config(capi.PRM_PRUNE_INVALID | capi.PRM_PRUNE_MASK), None, b"keep")
    refused(fake, _config(capi.PRM_PRUNE_INVALID), mask, b"OXHIP_PRM_PRUNE_MASK")
    refused(fake, _config(capi.PRM_PRUNE_LARGEST), mask, b"OXHIP_PRM_PRUNE_MASK")
    refused(fake, _config(capi.PRM_PRUNE_MIN_SIZE, min_size=0), None, b"min_size")
    refused(fake, _config(capi.PRM_PRUNE_MIN_SIZE | capi.PRM_PRUNE_MASK, min_size=0), mask, b"min_size")
    assert kept.value == 7 and removed.value == 7                       # a refused call writes nothing
    d = (C.c_double * 5)()
    launches = C.c_uint32()
    assert L.oxhip_prm_prune_last_timing(None, d) == capi.ERR_BAD_ARG
    assert L.oxhip_prm_components_last_timing(None, d, C.byref(launches)) == capi.ERR_BAD_ARG
    assert L.oxhip_prm_components(None, None, None, 0, None, None, None) == capi.ERR_BAD_ARG
    assert b"null" in L.oxhip_last_error_string()


def test_mirrors_have_the_surface():
    from oxmpl_amd.geometric import PRM
    for name in ("components", "components_timing", "prune", "prune_timing"):
        assert callable(getattr(capi.PRMRoadmap, name))
    assert callable(PRM.components) and callable(PRM.prune_roadmap)
    hpp = open(os.path.join(ROOT, "include", "oxmpl", "oxmpl.hpp")).read()
    rs = open(os.path.join(ROOT, "rust", "oxmpl-hip", "src", "lib.rs")).read()
    assert re.search(r"\bcomponents\(\)", hpp) and re.search(r"\bprune\(", hpp)
    assert "oxhip_prm_components(" in hpp and "oxhip_prm_prune(" in hpp and "oxhip_prm_prune_config" in hpp
    assert "pub fn components(" in rs and "pub fn prune(" in rs and "ffi::oxhip_prm_components(" in rs and "ffi::oxhip_prm_prune(" in rs
    for name, _ in FLAGS:
        assert "ffi::OXHIP_PRM_PRUNE_" + name in rs
    from oxmpl_amd.base import ProblemDefinition
    for call in (lambda p: p.components(), lambda p: p.prune_roadmap(largest=True)):
        with pytest.raises(Exception) as e:   # no setup(): the reference's message, before any library call
            call(PRM(1.0, 1.0, ProblemDefinition(None, None, None)))
        assert "setup() was not called" in str(e.value)


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "oxmpl/oxmpl.hpp"\n'
                   'int use(oxmpl::geometric::PRM& p) {\n'
                   '    auto c = p.components();\n'
                   '    std::vector<uint8_t> keep;\n'
                   '    auto r = p.prune(OXHIP_PRM_PRUNE_MASK | OXHIP_PRM_PRUNE_MIN_SIZE, 2, &keep);\n'
                   '    return p.last_prune_status() + (int)sizeof(c) + (int)sizeof(r);\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def _kernel_metadata(asm):
    meta = {}
    for block in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|"
                                                        r"group_segment_fixed_size|max_flat_workgroup_size):\s+(\d+)", block)}
    return meta


KERNELS = ["prm_cc_self_kernel", "prm_cc_init_kernel", "prm_cc_hook_kernel", "prm_cc_flatten_kernel", "prm_cc_count_kernel",
           "prm_cc_summary_kernel", "prm_prune_stage1_kernel", "prm_prune_stage2_kernel", "prm_prune_flags_kernel",
           "prm_prune_entries_kernel", "prm_prune_states_kernel"]


def test_prm_components_kernels_resource_shape(tmp_path):
    """Every kernel of prm_components.hip: 256-thread workgroups, private segment 0 (no scratch), both spill counts 0, no LDS."""
    out = str(tmp_path / "prm_components.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                           "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "prm_components.hip")], stderr=subprocess.DEVNULL)
    meta = _kernel_metadata(open(out).read())
    assert len(meta) == len(KERNELS) and all(sum(k in name for name in meta) == 1 for k in KERNELS), sorted(meta)
    misses = [(name, m) for name, m in meta.items()
              if not (m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0
                      and m["group_segment_fixed_size"] == 0 and m["max_flat_workgroup_size"] == 256)]
    assert not misses, misses


def test_new_kernels_live_in_their_own_file_and_the_makefile_builds_it():
    assert re.search(r"^SRCS\s*:=.*\bprm_components\.hip\b", open(os.path.join(CSRC, "Makefile")).read(), re.M)
    for other in ("prm_kernels.hip", "prm_batch.hip", "prm_shortest.hip", "prm_revalidate.hip", "prm_grow.hip", "path_simplify.hip", "shortcut_core.hip"):
        text = open(os.path.join(CSRC, other)).read()
        assert "prm_cc_" not in text and "prm_prune_" not in text, other
    # the hook kernel's forest is read and written through agent-scope atomics only: the find and the swap name them
    text = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "prm_components.hip")).read())   # (the code, not what the comments say)
    find = re.search(r"uint32_t cc_find\(.*?\n}\n", text, re.S).group(0)
    assert "ld_l2(" in find and "st_l2(" in find and not re.search(r"parent\[", find)
    hook = re.search(r"void prm_cc_hook_kernel\(.*?\n}\n", text, re.S).group(0)
    assert "__hip_atomic_compare_exchange_strong" in hook and "__HIP_MEMORY_SCOPE_AGENT" in hook and not re.search(r"parent\[", hook)
