"""CPU: the SO(3) additions to the C ABI (OXHIP_SPACE_SO3, oxhip_so3_op_batch) and to the Python surface.
(i)   an SO(3) RRT configuration passes the library's validation -- without a GPU, create() fails only for the missing device;
(ii)  the combinations that are not built, and the bounds SO3StateSpace::new rejects, are refused with BAD_ARG / ZERO_VOLUME;
(iii) the Python mirror classes build and refuse cleanly without a device;
(iv)  rrt_so3.hip compiles for gfx950 in the resource shape of the one-wave-per-problem kernels: no scratch, <= 40 KB of LDS,
      a 64-thread workgroup, and the tree / cone tables read through LDS or global instructions, never flat ones."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from oxmpl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oxmpl_amd", "csrc")
FIXTURE = [0.0, 0.0, 0.0, 1.0, math.pi]   # SO3StateSpace::new(None): identity centre, max_angle PI


@pytest.fixture(scope="module")
def L():
    capi.build_library()
    return capi.lib()


def _no_gpu(L):
    n = C.c_int32()
    return L.oxhip_device_count(C.byref(n)) != capi.OK


def _so3(**kw):
    args = dict(dim=4, bounds=FIXTURE, max_distance=0.5, goal_bias=0.0, n_problems=1, max_nodes=100, space=capi.SPACE_SO3)
    args.update(kw)
    return capi.RRTBatch(**args)


def test_so3_is_a_known_space_kind(L):
    """without a GPU the configuration reaches the device check: NO_DEVICE, not 'unknown space kind'"""
    if not _no_gpu(L):
        pytest.skip("a GPU is visible here")
    for kw in (dict(), dict(kernel=capi.KERNEL_STREAM), dict(bounds=[0.1, 0.2, 0.3, 0.9, 0.7]), dict(bounds=[0.0, 0.0, 0.0, 1.0, 9.0]),
               dict(bounds=[0.0, 0.0, 0.0, 1.0, float("nan")]), dict(goal_bias=0.05, lvs_fraction=0.01)):
        with pytest.raises(capi.OxhipError) as ei:
            _so3(**kw)
        assert ei.value.status == capi.ERR_NO_DEVICE, (kw, ei.value)
    with pytest.raises(capi.OxhipError) as ei:
        capi.so3_op_batch(0, np.zeros((1, 4)), np.ones((1, 4)))
    assert ei.value.status == capi.ERR_NO_DEVICE


@pytest.mark.parametrize("kw,code", [
    (dict(planner=capi.PLANNER_RRT_CONNECT), capi.ERR_BAD_ARG),
    (dict(planner=capi.PLANNER_RRT_STAR, search_radius=1.0), capi.ERR_BAD_ARG),
    (dict(kernel=capi.KERNEL_CELLS), capi.ERR_BAD_ARG),
    (dict(kernel=capi.KERNEL_LANES), capi.ERR_BAD_ARG),
    (dict(kernel=capi.KERNEL_RESIDENT), capi.ERR_BAD_ARG),
    (dict(goal_sampler=capi.GOAL_SAMPLE_UNIFORM_DISC), capi.ERR_BAD_ARG),
    (dict(bounds=[0.0, 0.0, 0.0, 1.0, -0.25]), capi.ERR_ZERO_VOLUME),         # StateSpaceError::InvalidAngularDistance
    (dict(bounds=[0.0, 0.0, 0.0, 1.0, -1e-300]), capi.ERR_ZERO_VOLUME),
    (dict(bounds=[0.0, 0.0, math.inf, 1.0, 1.0]), capi.ERR_BAD_ARG),          # centre not finite
    (dict(bounds=[0.0, 0.0, 1e200, 1.0, 1.0]), capi.ERR_BAD_ARG),             # ... or beyond 1e150
    (dict(lvs_fraction=0.0), capi.ERR_BAD_ARG),                               # check_motion would never end
    (dict(lvs_fraction=1e-9), capi.ERR_BAD_ARG),                              # > 1e6 validity checks per edge
    (dict(max_distance=0.0), capi.ERR_BAD_ARG),
    (dict(goal_bias=1.5), capi.ERR_BAD_ARG),
    (dict(bounds=[0.0, 0.0, 0.0, 1.0]), capi.ERR_BAD_ARG),                    # (the Python binding wants five values)
])
def test_so3_refuses_what_is_not_built_or_invalid(L, kw, code):
    with pytest.raises(capi.OxhipError) as ei:
        _so3(**kw)
    assert ei.value.status == code, ei.value


@pytest.mark.parametrize("dim", [2, 3, 5, 8])
def test_so3_states_are_four_wide(L, dim):
    cfg = capi.Config()
    cfg.struct_size, cfg.dim, cfg.space = C.sizeof(capi.Config), dim, capi.SPACE_SO3
    for i, v in enumerate(FIXTURE):
        cfg.bounds[i] = v
    cfg.max_distance, cfg.lvs_fraction, cfg.n_problems, cfg.max_nodes = 0.5, 0.05, 1, 100
    h = C.c_void_p()
    assert L.oxhip_rrt_batch_create(C.byref(cfg), C.byref(h)) == capi.ERR_BAD_ARG
    assert b"dim must be 4" in L.oxhip_last_error_string()


def test_unknown_space_kinds_stay_refused(L):
    with pytest.raises(capi.OxhipError) as ei:
        _so3(space=3)
    assert ei.value.status == capi.ERR_BAD_ARG


def test_so3_op_batch_rejects_bad_arguments(L):
    assert L.oxhip_so3_op_batch(0, 3, None, None, None, 1, None) == capi.ERR_BAD_ARG
    a = (C.c_double * 4)()
    out = (C.c_double * 4)()
    assert L.oxhip_so3_op_batch(0, 0, a, None, None, 1, out) == capi.ERR_BAD_ARG   # distance needs b
    assert L.oxhip_so3_op_batch(0, 1, a, a, None, 1, out) == capi.ERR_BAD_ARG      # interpolate needs t
    assert L.oxhip_so3_op_batch(0, 2, a, None, None, 0, out) == capi.OK            # nothing to do


def test_python_mirror_builds_and_refuses_without_a_device(L):
    from oxmpl_amd.base import ProblemDefinition, SO3ConeValidityChecker, SO3State, SO3StateSpace, SphereBoxValidityChecker
    from oxmpl_amd.geometric import RRT, RRTConnect

    class Goal:
        def __init__(self, target, radius):
            self.target, self.radius = target, radius

    space = SO3StateSpace()
    s = math.sqrt(0.5)
    start, target = SO3State(0.0, s, 0.0, s), SO3State(0.0, -s, 0.0, s)
    pd = ProblemDefinition.from_so3(space, start, Goal(target, math.radians(10.0)))
    checker = SO3ConeValidityChecker([(SO3State.identity(), math.radians(44.9))])
    assert checker.cones == [([0.0, 0.0, 0.0, 1.0], math.radians(44.9))]
    assert space.config_bounds() == FIXTURE
    assert repr(start).startswith("<SO3State x=0.0")
    with pytest.raises(TypeError):
        ProblemDefinition.from_so3(space, [0.0, 0.0, 0.0, 1.0], Goal(target, 0.1))
    with pytest.raises(ValueError):
        SO3ConeValidityChecker([([0.0, 0.0, 1.0], 0.1)])
    with pytest.raises(TypeError):   # the SO(3) problem takes cones, not spheres / boxes
        RRT(0.5, 0.0, pd).setup(SphereBoxValidityChecker())
    with pytest.raises(TypeError):   # RRTConnect on SO(3) is not built
        RRTConnect(0.5, 0.0, pd).setup(checker)
    with pytest.raises(ValueError):
        SO3StateSpace((SO3State.identity(), -0.5))
    if _no_gpu(L):
        with pytest.raises(capi.OxhipError) as ei:
            RRT(0.5, 0.0, pd).setup(checker)
        assert ei.value.status == capi.ERR_NO_DEVICE


def _kernels(asm):
    meta = {}
    for block in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|private_segment_fixed_size|"
                                                        r"group_segment_fixed_size|max_flat_workgroup_size):\s+(\d+)", block)}
    return meta


def test_rrt_so3_kernel_keeps_the_one_wave_shape(tmp_path):
    out = str(tmp_path / "rrt_so3.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                           "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "rrt_so3.hip")], stderr=subprocess.DEVNULL)
    asm = open(out).read()
    meta = {k: v for k, v in _kernels(asm).items() if "rrt_so3_kernel" in k}
    assert len(meta) == 2   # cone table in LDS / in HBM
    for name, m in meta.items():
        assert m["max_flat_workgroup_size"] == 64 and m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] <= 40960, (name, m)
        body = asm.split(name + ":")[1].split("s_endpgm")[0]
        assert "flat_load" not in body and "scratch_" not in body, name
        assert "ds_read" in body and "global_load" in body          # the LDS mirror and the nodes beyond it
        assert body.count("v_mul_f64") > 50 and body.count("v_add_f64") > 30   # unfused binary64 arithmetic
