"""CPU: the PRM / path kernels written once over SeqSpace<DIM> (oxmpl_amd/csrc/seq_space.hpp), compiled to gfx950 ISA (no GPU
needed): one kernel template per role, instantiated for R^1..R^8 and SO(3) (DIM = 0), no spill to scratch, no LDS, and no
instantiation needs more registers or spills more SGPRs than the hand-copied kernels it replaced.  The literals are the figures
of the commit before the trait, cross-compiled with the Makefile's flags; columns are D = 1..8, then SO(3), then SO(2)
(DIM = -1: the shortcut's kernels alone -- the pair matrix's figures are those of the commit before SO(2) joined space_dispatch --
and no PRM kernel).  The shortcut's pair matrix and DP exist once for the RRT and the PRM entry (shortcut_core.hip): the pair
matrix's two rows are its m = 1 and its subdivided instantiations ("kernel/flag" names the template's bool argument), held to the
figures of the two kernels they replaced, and the DP is held to the subdivided DP's, SO(2) to R^1's (one double per state)."""
import os
import re
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, _kernels

SOURCES = ["prm_kernels.hip", "prm_batch.hip", "prm_revalidate.hip", "shortcut_core.hip", "prm_shortest.hip"]
DIMS = [1, 2, 3, 4, 5, 6, 7, 8, 0, -1]

# kernel -> (vgpr_count, sgpr_spill_count) per D of DIMS; None: no such instantiation (no caller reaches it)
BEFORE = {
    "prm_query_kernel": ([28, 36, 46, 56, 66, 76, 86, 97, 85, None], [0, 0, 0, 4, 8, 47, 73, 117, 16, None]),
    "prm_batch_flags_kernel": ([28, 36, 46, 56, 66, 76, 87, 97, 85, None], [0, 0, 0, 8, 35, 58, 102, 122, 24, None]),
    "prm_reval_valid_kernel": ([18, 26, 32, 38, 44, 44, 60, 68, 40, None], [0] * 9 + [None]),
    "prm_reval_check_kernel": ([40, 48, 58, 68, 78, 88, 98, 110, None, None], [0] * 8 + [None, None]),   # SO(3) re-checks through prm_so3_edge_kernel
    "shortcut_pairs_kernel/Lb0": ([None, 36, 46, 56, 66, 77, 87, 97, 93, 40], [None, 0, 0, 0, 0, 11, 30, 64, 6, 0]),   # an RRT batch has dim >= 2
    "shortcut_pairs_kernel/Lb1": ([30, 38, 46, 58, 66, 77, 87, 98, 93, None], [0, 0, 0, 0, 0, 15, 40, 68, 8, None]),
    "shortcut_dp_kernel": ([27, 29, 31, 33, 36, 40, 44, 48, 50, 27], [0] * 10),
    "prm_shortest_weights_kernel": ([12, 14, 18, 22, 26, 30, 34, 38, 24, None], [0] * 9 + [None]),
    "prm_shortest_init_kernel": ([12, 12, 12, 12, 15, 16, 19, 20, 24, None], [0] * 9 + [None]),
}


@pytest.fixture(scope="module")
def trait_kernels(tmp_path_factory):
    """mangled name -> metadata of every kernel of the five sources (compiled side by side)"""
    d = tmp_path_factory.mktemp("asm_space_trait")
    procs = []
    for src in SOURCES:
        out = str(d / (src[:-4] + ".s"))
        procs.append((out, subprocess.Popen([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                                             "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, src)], stderr=subprocess.DEVNULL)))
    meta = {}
    for out, p in procs:
        assert p.wait() == 0, out
        meta.update(_kernels(open(out).read()))
    return meta


def _instantiations(meta, kernel):
    """D -> metadata of kernel<D>, or of kernel<D, flag> for "kernel/flag"  (a negative D mangles as n<digits>: -1 is ILin1E)"""
    kernel, _, flag = kernel.partition("/")
    found = {}
    for name, m in meta.items():
        hit = re.search(r"\d+" + kernel + r"ILi(n?)(\d+)E" + flag + "EE", name)
        if hit:
            d = -int(hit.group(2)) if hit.group(1) else int(hit.group(2))
            assert d not in found, name
            found[d] = m
    return found


@pytest.mark.parametrize("kernel", sorted(BEFORE))
def test_one_template_per_role_within_the_figures_before_the_trait(trait_kernels, kernel):
    vgpr, spill = BEFORE[kernel]
    inst = _instantiations(trait_kernels, kernel)
    assert sorted(inst) == sorted(d for d, v in zip(DIMS, vgpr) if v is not None)      # exactly these instantiations (see BEFORE)
    for d, v, s in zip(DIMS, vgpr, spill):
        if v is None:
            continue
        m = inst[d]
        assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0 and m["group_segment_fixed_size"] == 0, (kernel, d, m)
        assert m["vgpr_count"] <= v and m["sgpr_spill_count"] <= s, (kernel, d, m, v, s)
        if kernel.startswith("prm_reval"):
            assert m["sgpr_spill_count"] == 0, (kernel, d, m)                          # the obstacle tables' pointers travel in VGPRs


def test_no_hand_copied_so3_twin_is_left(trait_kernels):
    for name in trait_kernels:
        for gone in ("so3_query", "so3_flags", "so3_valid", "pairs_so3", "path_pairs_kernel", "path_dp_kernel", "dense_pairs_kernel", "dense_dp_kernel"):
            assert gone not in name, name
    for kernel in BEFORE:   # and no second kernel of the role under another name: every symbol of the role is the template's
        base, _, flag = kernel.partition("/")
        names = [n for n in trait_kernels if base in n and flag in n]
        assert len(names) == len(_instantiations(trait_kernels, kernel)), names
