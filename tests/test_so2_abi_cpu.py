"""CPU: the SO(2) additions to the C ABI (OXHIP_SPACE_SO2 = 16) and to the Python surface.
(i)   a valid SO(2) RRT configuration passes the library's validation -- without a GPU, create() fails only for the missing
      device, not as an unknown space kind;
(ii)  the combinations that are not built and the bounds SO2StateSpace::new rejects are refused with their codes; the kinds
      4 .. 15 and 17 stay unknown, and PRM keeps refusing kind 16;
(iii) the Python mirror classes build, normalise and refuse without a device; the Rust crate carries the constant;
(iv)  rrt_so2.hip compiles for gfx950 in the resource shape of the one-wave-per-problem kernels, read from the code object's
      metadata: a 64-thread workgroup, at most 40 KB of LDS, no scratch, no spills, both instantiations."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest

from oxmpl_amd import capi

import so2_helpers as h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oxmpl_amd", "csrc")
PI = math.pi


@pytest.fixture(scope="module")
def L():
    capi.build_library()
    return capi.lib()


def _no_gpu(L):
    n = C.c_int32()
    return L.oxhip_device_count(C.byref(n)) != capi.OK


def _so2(**kw):
    args = dict(dim=1, bounds=[-PI, PI], max_distance=0.2, goal_bias=0.05, n_problems=1, max_nodes=100, space=capi.SPACE_SO2,
                planner=capi.PLANNER_RRT)
    args.update(kw)
    return capi.RRTBatch(**args)


def test_constants(L):
    assert capi.SPACE_SO2 == 16 and capi.ABI_VERSION == 2 and L.oxhip_abi_version() == 2
    hdr = open(os.path.join(ROOT, "include", "oxmpl_hip.h")).read()
    assert re.search(r"OXHIP_SPACE_SO2\s*=\s*16\b", hdr)
    ffi = open(os.path.join(ROOT, "rust", "oxmpl-hip", "src", "ffi.rs")).read()
    assert "OXHIP_SPACE_SO2: u32 = 16" in ffi
    lib_rs = open(os.path.join(ROOT, "rust", "oxmpl-hip", "src", "lib.rs")).read()
    assert "fn so2_rrt_config(" in lib_rs


def test_kernel_constants_are_read_from_the_source():
    assert h.K_SO2_N == 4096 and h.K_SO2_LDS_ARCS == 64
    assert h.K_SO2_N * 8 + 4096 + 2 * 64 * 8 + 2 * 8 * h.K_SO2_LDS_ARCS <= 40960   # mirror, RNG window, sample block, arcs


@pytest.mark.parametrize("kw", [
    dict(), dict(bounds=[-9.0, 9.0]), dict(bounds=[-1.0, 2.0]), dict(kernel=capi.KERNEL_STREAM), dict(goal_bias=1.0, lvs_fraction=0.01),
    dict(lvs_fraction=7.0), dict(n_problems=1024, max_nodes=10000), dict(max_distance=10.0),
])
def test_so2_is_a_known_space_kind(L, kw):
    """a valid configuration reaches the device: created where there is one, NO_DEVICE -- not 'unknown space kind' -- where not"""
    if _no_gpu(L):
        with pytest.raises(capi.OxhipError) as ei:
            _so2(**kw)
        assert ei.value.status == capi.ERR_NO_DEVICE, (kw, ei.value)
    else:
        _so2(**kw).close()


@pytest.mark.parametrize("kw,code,msg", [
    (dict(dim=2, bounds=[-PI, PI, 0.0, 1.0]), capi.ERR_BAD_ARG, "dim must be 1"),
    (dict(dim=3, bounds=[-PI, PI] * 3), capi.ERR_BAD_ARG, "dim must be 1"),
    (dict(planner=capi.PLANNER_RRT_CONNECT), capi.ERR_BAD_ARG, "SO(2) is built for RRT only"),
    (dict(planner=capi.PLANNER_RRT_STAR, search_radius=1.0), capi.ERR_BAD_ARG, "SO(2) is built for RRT only"),
    (dict(kernel=capi.KERNEL_CELLS), capi.ERR_BAD_ARG, "rrt_so2.hip"),
    (dict(kernel=capi.KERNEL_LANES), capi.ERR_BAD_ARG, "rrt_so2.hip"),
    (dict(kernel=capi.KERNEL_RESIDENT), capi.ERR_BAD_ARG, "rrt_so2.hip"),
    (dict(goal_sampler=capi.GOAL_SAMPLE_UNIFORM_DISC), capi.ERR_BAD_ARG, "disc sampler"),
    (dict(bounds=[1.0, 1.0]), capi.ERR_ZERO_VOLUME, "lower bound >= upper bound"),       # SO2StateSpace::new: InvalidBound
    (dict(bounds=[2.0, -2.0]), capi.ERR_ZERO_VOLUME, "lower bound >= upper bound"),
    (dict(bounds=[math.nan, 1.0]), capi.ERR_ZERO_VOLUME, "lower bound >= upper bound"),  # a NaN bound: refused too
    (dict(bounds=[-1.0, math.nan]), capi.ERR_ZERO_VOLUME, "lower bound >= upper bound"),
    (dict(lvs_fraction=0.0), capi.ERR_BAD_ARG, "longest valid segment length is 0"),      # check_motion would never end
    (dict(lvs_fraction=-1.0), capi.ERR_BAD_ARG, "longest valid segment length is 0"),
    (dict(lvs_fraction=1e-9), capi.ERR_BAD_ARG, "1e6"),                                   # > 1e6 validity checks per edge
    (dict(max_distance=0.0), capi.ERR_BAD_ARG, ""),
    (dict(goal_bias=1.5), capi.ERR_BAD_ARG, ""),
    (dict(bounds=[-PI, PI, 0.0]), capi.ERR_BAD_ARG, "bounds"),                            # (the Python binding wants dim pairs)
])
def test_so2_refuses_what_is_not_built_or_invalid(L, kw, code, msg):
    with pytest.raises(capi.OxhipError) as ei:
        _so2(**kw)
    assert ei.value.status == code and msg in str(ei.value), ei.value


@pytest.mark.parametrize("space", list(range(4, 16)) + [17, 32, 0xFFFFFFFF])
def test_other_space_kinds_stay_unknown(L, space):
    for dim in (1, 3):
        cfg = capi.Config()
        cfg.struct_size, cfg.dim, cfg.space, cfg.planner = C.sizeof(capi.Config), dim, space, capi.PLANNER_RRT
        for i in range(2 * dim):
            cfg.bounds[i] = (-1.0, 1.0)[i % 2]
        cfg.max_distance, cfg.lvs_fraction, cfg.n_problems, cfg.max_nodes = 0.2, 0.05, 1, 100
        handle = C.c_void_p()
        assert L.oxhip_rrt_batch_create(C.byref(cfg), C.byref(handle)) == capi.ERR_BAD_ARG
        assert b"unknown space kind" in L.oxhip_last_error_string()


def test_prm_keeps_refusing_kind_16(L):
    with pytest.raises(capi.OxhipError) as so2_err:
        capi.PRMRoadmap(1, [(-PI, PI)], 1.0, 100, space=capi.SPACE_SO2)
    with pytest.raises(capi.OxhipError) as se3_err:
        capi.PRMRoadmap(7, [(-5.0, 5.0)] * 7, 1.0, 100, space=capi.SPACE_SE3)
    assert so2_err.value.status == capi.ERR_BAD_ARG and "PRM space" in str(so2_err.value)
    assert str(so2_err.value) == str(se3_err.value)   # the text it uses for SE(3)


def test_python_mirror_builds_normalises_and_refuses_without_a_device(L):
    from oxmpl_amd import scenarios
    from oxmpl_amd.base import (ProblemDefinition, SO2ArcValidityChecker, SO2State, SO2StateSpace, SO3StateSpace,
                                SphereBoxValidityChecker)
    from oxmpl_amd.geometric import PRM, RRT, RRTConnect, RRTStar

    class Goal:
        def __init__(self, target, radius):
            self.target, self.radius = target, radius

    assert SO2State(1.0).value == 1.0 and SO2State(1.0).values == [1.0]
    assert abs(SO2State(5.0 * PI).value + PI) < 1e-9 and abs(SO2State(3.0 * PI / 2.0).value + PI / 2.0) < 1e-9   # so2_state.rs doctests
    assert SO2State(PI).value == -PI and SO2State(-PI).value == -PI and SO2State(0.0) == SO2State(0.0)
    assert [SO2State(v).value for v in (-7.0, 50.0, -1e6)] == [h.so2.normalise(v) for v in (-7.0, 50.0, -1e6)]
    space = SO2StateSpace()
    assert space.bounds == (-PI, PI) and space.dimension == 1 and space.longest_valid_segment_fraction == 0.05
    assert space.get_maximum_extent() == PI and space.config_bounds() == [-PI, PI]
    assert SO2StateSpace((0.0, PI)).bounds == (0.0, PI) and SO2StateSpace((-9.0, 9.0)).bounds == (-PI, PI)
    for bad in ((1.0, 1.0), (2.0, -2.0), (math.nan, 1.0)):
        with pytest.raises(ValueError):
            SO2StateSpace(bad)
    assert space.distance(SO2State(3.0), SO2State(-3.0)) == h.so2.distance(3.0, -3.0) < 0.3   # across the seam
    space.set_longest_valid_segment_fraction(7.0)
    assert space.longest_valid_segment_fraction == 1.0
    space.set_longest_valid_segment_fraction(-1.0)
    assert space.longest_valid_segment_fraction == 0.0
    space.set_longest_valid_segment_fraction(0.05)
    checker = SO2ArcValidityChecker([(-0.5, 0.5), (1, 2)])
    assert checker.arcs == [(-0.5, 0.5), (1.0, 2.0)]
    start, target = SO2State(-PI / 2.0), SO2State(PI / 2.0)
    pd = ProblemDefinition.from_so2(space, start, Goal(target, 0.1))
    with pytest.raises(TypeError):
        ProblemDefinition.from_so2(space, -1.0, Goal(target, 0.1))
    with pytest.raises(TypeError):
        ProblemDefinition.from_so2(SO3StateSpace(), start, Goal(target, 0.1))
    with pytest.raises(TypeError):
        ProblemDefinition.from_so2(space, start, object())
    with pytest.raises(TypeError):   # an SO(2) problem takes arcs
        RRT(0.2, 0.05, pd).setup(SphereBoxValidityChecker())
    with pytest.raises(TypeError):   # RRTConnect, RRT* and PRM over SO(2) are not built
        RRTConnect(0.2, 0.05, pd).setup(checker)
    with pytest.raises(TypeError):
        RRTStar(0.2, 0.05, 1.0, pd).setup(checker)
    with pytest.raises(TypeError):
        PRM(1.0, 0.5, pd).setup(checker)
    sc = scenarios.so2_band()
    assert sc["start"] == [h.so2.fixture_scene()["start"]] and sc["arcs"] == h.so2.fixture_scene()["arcs"]
    if _no_gpu(L):
        with pytest.raises(capi.OxhipError) as ei:
            RRT(0.2, 0.05, pd).setup(checker)
        assert ei.value.status == capi.ERR_NO_DEVICE
        with pytest.raises(capi.OxhipError) as ei:
            scenarios.make_so2_batch(sc, 4)
        assert ei.value.status == capi.ERR_NO_DEVICE
    else:
        RRT(0.2, 0.05, pd).setup(checker)


def test_the_other_checkers_are_refused_with_a_text_that_names_arcs(L):
    if _no_gpu(L):
        src = open(os.path.join(CSRC, "oxhip_api.hip")).read()   # (the calls need a batch; without a device: the table's row)
        row = src.split("/* OXHIP_SPACE_SO2 */")[1].split("},")[0]
        assert "kSo2Arcs, nullptr, kSo2Arcs, kSo2Arcs" in row and "forbidden arcs" in src.split("kSo2Arcs =")[1].split(";")[0]
        return
    b = _so2()
    for call in (lambda: b.set_spheres([[0.0]], [0.1]), lambda: b.set_segments([[0.0, 0.0, 1.0, 1.0]], 0.1),
                 lambda: b.set_body([[0.0] * 3], [0.1])):
        with pytest.raises(capi.OxhipError) as ei:
            call()
        assert ei.value.status == capi.ERR_BAD_ARG and "arcs" in str(ei.value)
    b.close()


def _kernels(asm):
    meta = {}
    for block in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|"
                                                        r"group_segment_fixed_size|max_flat_workgroup_size):\s+(\d+)", block)}
    return meta


def test_rrt_so2_kernel_keeps_the_one_wave_shape(tmp_path):
    out = str(tmp_path / "rrt_so2.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                           "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "rrt_so2.hip")], stderr=subprocess.DEVNULL)
    every = _kernels(open(out).read())
    meta = {k: v for k, v in every.items() if "rrt_so2_kernel" in k}
    assert len(meta) == 2 and sum("ILb1E" in k for k in meta) == 1 and sum("ILb0E" in k for k in meta) == 1   # arcs in LDS / in HBM
    for name, m in meta.items():
        assert m["max_flat_workgroup_size"] == 64 and m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] <= 40960, (name, m)          # four problems per CU
    lds = {("ILb1E" in k): v["group_segment_fixed_size"] for k, v in meta.items()}
    assert lds[True] - lds[False] == 2 * 8 * (h.K_SO2_LDS_ARCS - 1)      # the HBM instantiation stages no arc table
    assert lds[False] >= 8 * h.K_SO2_N + 4096                            # the mirror and the RNG window
    for name in ("so2_is_valid_kernel", "so2_check_motion_kernel"):
        ms = [v for k, v in every.items() if name in k]
        assert len(ms) == 1 and ms[0]["private_segment_fixed_size"] == 0 and ms[0]["vgpr_spill_count"] == 0, (name, ms)
