"""CPU: the SE(3) additions to the C ABI (OXHIP_SPACE_SE3, oxhip_rrt_batch_set_body, oxhip_se3_op_batch) and to the Python surface.
(i)   a valid SE(3) RRTConnect configuration passes the library's validation -- without a GPU, create() fails only for the
      missing device, not as an unknown space kind;
(ii)  the combinations that are not built, and the bounds the component spaces reject, are refused with their codes;
(iii) set_body / se3_op_batch check their arguments;
(iv)  the Python mirror classes build, convert and refuse without a device;
(v)   rrt_connect_se3.hip compiles for gfx950 in the resource shape of the one-wave-per-problem kernels: a 64-thread workgroup,
      at most 40 KB of LDS, no scratch, no spills, no flat loads, unfused binary64 arithmetic; and rrt_so3.hip, whose sampler moved
      into a shared header, still holds its two kernels."""
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
BOUNDS = [-5.0, 5.0] * 3 + [0.0, 0.0, 0.0, 1.0, math.pi]   # [-5, 5]^3, every rotation


@pytest.fixture(scope="module")
def L():
    capi.build_library()
    return capi.lib()


def _no_gpu(L):
    n = C.c_int32()
    return L.oxhip_device_count(C.byref(n)) != capi.OK


def _se3(**kw):
    args = dict(dim=7, bounds=BOUNDS, max_distance=1.0, goal_bias=0.05, n_problems=1, max_nodes=100, space=capi.SPACE_SE3,
                planner=capi.PLANNER_RRT_CONNECT)
    args.update(kw)
    return capi.RRTBatch(**args)


def _bounds(**kw):
    b = list(BOUNDS)
    for i, v in kw.items():
        b[int(i[1:])] = v
    return b


def test_constants_and_exports(L):
    assert capi.SPACE_SE3 == 3 and capi.ABI_VERSION == 2 and C.sizeof(capi.Config) == 232
    hdr = open(os.path.join(ROOT, "include", "oxmpl_hip.h")).read()
    assert re.search(r"OXHIP_SPACE_SE3\s*=\s*3\b", hdr)
    for name in ("oxhip_rrt_batch_set_body", "oxhip_se3_op_batch"):
        assert name in capi.EXPORTS and hasattr(L, name) and (name + "(") in hdr
    ffi = open(os.path.join(ROOT, "rust", "oxmpl-hip", "src", "ffi.rs")).read()
    assert "OXHIP_SPACE_SE3: u32 = 3" in ffi and "fn oxhip_rrt_batch_set_body(" in ffi and "fn oxhip_se3_op_batch(" in ffi


@pytest.mark.parametrize("kw", [
    dict(), dict(kernel=capi.KERNEL_STREAM), dict(bounds=_bounds(b6=0.1, b7=0.2, b8=-0.3, b9=0.9, b10=1.2)),
    dict(bounds=_bounds(b10=9.0)), dict(bounds=_bounds(b10=float("nan"))), dict(goal_bias=1.0, lvs_fraction=0.01),
    dict(bounds=[0.0, 1e6, -3.0, 2.0, 1e-3, 2e-3, 0.0, 0.0, 0.0, 1.0, 0.0]), dict(n_problems=1024, max_nodes=10000),
])
def test_se3_is_a_known_space_kind(L, kw):
    """a valid configuration reaches the device: it is created where there is one, and NO_DEVICE -- not 'unknown space kind' --
    where there is none"""
    if _no_gpu(L):
        with pytest.raises(capi.OxhipError) as ei:
            _se3(**kw)
        assert ei.value.status == capi.ERR_NO_DEVICE, (kw, ei.value)
    else:
        _se3(**kw).close()


@pytest.mark.parametrize("kw,code,msg", [
    (dict(planner=capi.PLANNER_RRT), capi.ERR_BAD_ARG, "RRTConnect"),
    (dict(planner=capi.PLANNER_RRT_STAR, search_radius=1.0), capi.ERR_BAD_ARG, "RRTConnect"),
    (dict(kernel=capi.KERNEL_CELLS), capi.ERR_BAD_ARG, ""),
    (dict(kernel=capi.KERNEL_LANES), capi.ERR_BAD_ARG, ""),
    (dict(kernel=capi.KERNEL_RESIDENT), capi.ERR_BAD_ARG, ""),
    (dict(goal_sampler=capi.GOAL_SAMPLE_UNIFORM_DISC), capi.ERR_BAD_ARG, ""),
    (dict(bounds=_bounds(b1=math.inf)), capi.ERR_UNBOUNDED, "unbounded"),             # RealVectorStateSpace::new(3, ..)
    (dict(bounds=_bounds(b4=-math.inf)), capi.ERR_UNBOUNDED, "unbounded"),
    (dict(bounds=_bounds(b2=5.0)), capi.ERR_ZERO_VOLUME, ""),                         # lo >= hi
    (dict(bounds=_bounds(b0=6.0)), capi.ERR_ZERO_VOLUME, ""),
    (dict(bounds=_bounds(b10=-0.25)), capi.ERR_ZERO_VOLUME, "max_angle"),             # SO3StateSpace::new
    (dict(bounds=_bounds(b10=-1e-300)), capi.ERR_ZERO_VOLUME, "max_angle"),
    (dict(bounds=_bounds(b8=math.inf)), capi.ERR_BAD_ARG, "centre"),                  # rotation centre not finite
    (dict(bounds=_bounds(b6=1e200)), capi.ERR_BAD_ARG, "centre"),
    (dict(lvs_fraction=0.0), capi.ERR_BAD_ARG, ""),                                   # check_motion would never end
    (dict(lvs_fraction=1e-9), capi.ERR_BAD_ARG, "1e6"),                               # > 1e6 validity checks per edge
    (dict(max_distance=0.0), capi.ERR_BAD_ARG, ""),
    (dict(goal_bias=1.5), capi.ERR_BAD_ARG, ""),
    (dict(bounds=BOUNDS[:10]), capi.ERR_BAD_ARG, "SE(3) bounds"),                     # (the Python binding wants eleven values)
    (dict(bounds=[-5.0, 5.0] * 7), capi.ERR_BAD_ARG, "SE(3) bounds"),
])
def test_se3_refuses_what_is_not_built_or_invalid(L, kw, code, msg):
    with pytest.raises(capi.OxhipError) as ei:
        _se3(**kw)
    assert ei.value.status == code and msg in str(ei.value), ei.value


@pytest.mark.parametrize("dim", [3, 4, 6, 8])
def test_se3_states_are_seven_wide(L, dim):
    for planner in (capi.PLANNER_RRT, capi.PLANNER_RRT_CONNECT):
        cfg = capi.Config()
        cfg.struct_size, cfg.dim, cfg.space, cfg.planner = C.sizeof(capi.Config), dim, capi.SPACE_SE3, planner
        for i, v in enumerate(BOUNDS):
            cfg.bounds[i] = v
        cfg.max_distance, cfg.lvs_fraction, cfg.n_problems, cfg.max_nodes = 1.0, 0.05, 1, 100
        h = C.c_void_p()
        assert L.oxhip_rrt_batch_create(C.byref(cfg), C.byref(h)) == capi.ERR_BAD_ARG
        assert b"dim must be 7" in L.oxhip_last_error_string()


def test_space_kinds_beyond_se3_and_prm_over_se3_stay_refused(L):
    with pytest.raises(capi.OxhipError) as ei:
        _se3(space=4, bounds=[-5.0, 5.0] * 7)
    assert ei.value.status == capi.ERR_BAD_ARG and "unknown space kind" in str(ei.value)
    with pytest.raises(capi.OxhipError) as ei:
        capi.PRMRoadmap(7, [(-5.0, 5.0)] * 7, 1.0, 100, space=capi.SPACE_SE3)
    assert ei.value.status == capi.ERR_BAD_ARG and "PRM space" in str(ei.value)


def test_set_body_and_se3_op_batch_check_their_arguments(L):
    c3, r1 = (C.c_double * 3)(), (C.c_double * 1)()
    assert L.oxhip_rrt_batch_set_body(None, c3, r1, 1) == capi.ERR_BAD_ARG          # null batch
    a, out = (C.c_double * 7)(), (C.c_double * 7)()
    assert L.oxhip_se3_op_batch(0, 3, a, a, None, 1, out) == capi.ERR_BAD_ARG       # unknown op
    assert L.oxhip_se3_op_batch(0, 0, None, a, None, 1, out) == capi.ERR_BAD_ARG
    assert L.oxhip_se3_op_batch(0, 0, a, None, None, 1, out) == capi.ERR_BAD_ARG
    assert L.oxhip_se3_op_batch(0, 0, a, a, None, 1, None) == capi.ERR_BAD_ARG
    assert L.oxhip_se3_op_batch(0, 1, a, a, None, 1, out) == capi.ERR_BAD_ARG       # interpolate needs t
    assert L.oxhip_se3_op_batch(0, 2, a, a, None, 0, out) == capi.OK                # nothing to do
    if _no_gpu(L):
        with pytest.raises(capi.OxhipError) as ei:
            capi.se3_op_batch(0, np.zeros((1, 7)), np.ones((1, 7)))
        assert ei.value.status == capi.ERR_NO_DEVICE
        return
    # with a device: the refusals that need a batch
    b = _se3()
    for centres, radii in (([[0.0] * 3] * 17, [0.1] * 17), ([[0.0] * 3], [-0.1]), ([[0.0] * 3], [math.inf]), ([[0.0] * 3], [math.nan]),
                           ([[math.nan, 0.0, 0.0]], [0.1]), ([[0.0, math.inf, 0.0]], [0.1])):
        with pytest.raises(capi.OxhipError) as ei:
            b.set_body(centres, radii)
        assert ei.value.status == capi.ERR_BAD_ARG, (centres, radii)
    assert L.oxhip_rrt_batch_set_body(b._h, c3, r1, 0) == capi.ERR_BAD_ARG          # an empty body
    b.set_body([[0.0] * 3] * 16, [0.1] * 16)
    with pytest.raises(capi.OxhipError) as ei:
        b.set_boxes([[0.0] * 7], [[1.0] * 7])
    assert ei.value.status == capi.ERR_BAD_ARG
    with pytest.raises(capi.OxhipError) as ei:
        b.set_segments([[0.0, 0.0, 1.0, 1.0]], 0.1)
    assert ei.value.status == capi.ERR_BAD_ARG
    b.close()
    r3 = capi.RRTBatch(3, [(0.0, 1.0)] * 3, 0.5, 0.05, 1, 100)                        # a body belongs to SE(3) batches only
    with pytest.raises(capi.OxhipError) as ei:
        r3.set_body([[0.0] * 3], [0.1])
    assert ei.value.status == capi.ERR_BAD_ARG
    r3.close()


def test_python_mirror_builds_converts_and_refuses_without_a_device(L):
    from oxmpl_amd.base import (ProblemDefinition, SE3RigidBodyValidityChecker, SE3State, SE3StateSpace, SO3State, SO3StateSpace,
                                SphereBoxValidityChecker)
    from oxmpl_amd.geometric import RRT, RRTConnect, RRTStar

    class Goal:
        def __init__(self, target, radius):
            self.target, self.radius = target, radius

    h = math.sqrt(0.5)
    start = SE3State(-4.0, -4.0, -4.0, SO3State(0.0, h, 0.0, h))
    target = SE3State.from_values([4.0, 4.0, 4.0, 0.0, -h, 0.0, h])
    assert start.values == [-4.0, -4.0, -4.0, 0.0, h, 0.0, h] and target.rotation == SO3State(0.0, -h, 0.0, h)
    assert SE3State.from_values(start.values) == start and repr(start).startswith("<SE3State x=-4.0")
    with pytest.raises(TypeError):
        SE3State(0.0, 0.0, 0.0, [0.0, 0.0, 0.0, 1.0])
    with pytest.raises(ValueError):
        SE3State.from_values([0.0] * 6)
    space = SE3StateSpace([(-5.0, 5.0)] * 3)
    assert space.dimension == 7 and space.longest_valid_segment_fraction == 0.05
    assert space.config_bounds() == BOUNDS
    tilt = SE3StateSpace([(0.0, 1.0), (0.0, 2.0), (-1.0, 3.0)], (SO3State(0.0, 0.6, 0.0, 0.8), 1.2))
    assert tilt.config_bounds() == [0.0, 1.0, 0.0, 2.0, -1.0, 3.0, 0.0, 0.6, 0.0, 0.8, 1.2]
    space.set_longest_valid_segment_fraction(7.0)
    assert space.longest_valid_segment_fraction == 1.0
    space.set_longest_valid_segment_fraction(0.05)
    with pytest.raises(ValueError):
        SE3StateSpace([(-5.0, 5.0)] * 2)
    with pytest.raises(ValueError):
        SE3StateSpace([(-5.0, 5.0)] * 3, (SO3State.identity(), -0.5))
    checker = SE3RigidBodyValidityChecker([([-1.0, 0.0, 0.0], 0.25), ([1.0, 0.0, 0.0], 0.25)], [([0.0, 0.0, 0.0], 1.0)])
    assert checker.body == [([-1.0, 0.0, 0.0], 0.25), ([1.0, 0.0, 0.0], 0.25)] and checker.obstacles == [([0.0, 0.0, 0.0], 1.0)]
    assert SE3RigidBodyValidityChecker().body == [([0.0, 0.0, 0.0], 0.0)]          # a point
    for bad in (dict(body=[]), dict(body=[([0.0] * 3, 0.1)] * 17), dict(body=[([0.0] * 3, -0.1)]), dict(body=[([0.0] * 2, 0.1)]),
                dict(obstacles=[([0.0] * 4, 0.1)])):
        with pytest.raises(ValueError):
            SE3RigidBodyValidityChecker(**bad)
    pd = ProblemDefinition.from_se3(space, start, Goal(target, 0.25))
    with pytest.raises(TypeError):
        ProblemDefinition.from_se3(space, start.values, Goal(target, 0.25))
    with pytest.raises(TypeError):
        ProblemDefinition.from_se3(SO3StateSpace(), start, Goal(target, 0.25))
    with pytest.raises(TypeError):
        ProblemDefinition.from_se3(space, start, object())
    with pytest.raises(TypeError):   # the SE(3) problem takes a rigid body, not spheres / boxes
        RRTConnect(1.0, 0.05, pd).setup(SphereBoxValidityChecker())
    with pytest.raises(TypeError):   # RRT and RRT* over SE(3) are not built
        RRT(1.0, 0.05, pd).setup(checker)
    with pytest.raises(TypeError):
        RRTStar(1.0, 0.05, 1.0, pd).setup(checker)
    if _no_gpu(L):
        with pytest.raises(capi.OxhipError) as ei:
            RRTConnect(1.0, 0.05, pd).setup(checker)
        assert ei.value.status == capi.ERR_NO_DEVICE
        with pytest.raises(capi.OxhipError) as ei:
            space.distance(start, target)
        assert ei.value.status == capi.ERR_NO_DEVICE
    else:
        RRTConnect(1.0, 0.05, pd).setup(checker)


def _kernels(asm):
    meta = {}
    for block in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|"
                                                        r"group_segment_fixed_size|max_flat_workgroup_size):\s+(\d+)", block)}
    return meta


def _asm(tmp_path, src):
    out = str(tmp_path / (src + ".s"))
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                           "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, src)], stderr=subprocess.DEVNULL)
    return open(out).read()


def test_rrt_connect_se3_kernel_keeps_the_one_wave_shape(tmp_path):
    asm = _asm(tmp_path, "rrt_connect_se3.hip")
    meta = {k: v for k, v in _kernels(asm).items() if "rrt_connect_se3_kernel" in k}
    assert len(meta) == 4   # obstacles in LDS / in HBM, each as the product and as the stamped diagnostic instantiation
    for name, m in meta.items():
        assert m["max_flat_workgroup_size"] == 64 and m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] <= 40960, (name, m)          # four problems per CU
        assert m["vgpr_count"] <= 256, (name, m)
        if "Lb1EEEv" in name:   # the stamped diagnostic instantiation (second template argument): resources only
            continue
        body = asm.split(name + ":")[1].split("s_endpgm")[0]
        assert "flat_load" not in body and "flat_store" not in body and "scratch_" not in body, name
        assert "ds_read" in body and "global_load" in body               # the LDS mirrors and the nodes beyond them
        assert body.count("v_mul_f64") > 50 and body.count("v_add_f64") > 50   # unfused binary64 arithmetic
        assert "_dpp" in body                                            # the wave minimum runs on the DPP crossbar, not through LDS
    assert sum("Lb0EEEv" in k for k in meta) == 2
    lds = {("ILb1E" in k): v["group_segment_fixed_size"] for k, v in meta.items()}   # (the first template argument: LDS_OBS)
    assert lds[True] > lds[False]                                        # the HBM instantiation stages no obstacle table
    for name, m in _kernels(asm).items():                                # the stand-alone hooks too: no scratch anywhere in the file
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)


def test_rrt_so3_still_holds_its_two_kernels(tmp_path):
    asm = _asm(tmp_path, "rrt_so3.hip")
    meta = {k: v for k, v in _kernels(asm).items() if "rrt_so3_kernel" in k}
    assert len(meta) == 2
    src = open(os.path.join(CSRC, "rrt_so3.hip")).read()
    assert '#include "so3_sampler.hpp"' in src and "so3_sample_uniform_wave" in src
    assert "so3_sample_uniform_wave" in open(os.path.join(CSRC, "rrt_connect_se3.hip")).read()   # one sampler, two kernels
