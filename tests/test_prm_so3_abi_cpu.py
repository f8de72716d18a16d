"""CPU: the SO(3) mode of the PRM ABI (oxhip_prm_config.space = OXHIP_SPACE_SO3, prm_so3.hip) and of the Python surface.
(i)   SO(3) PRM configurations pass the library's validation: without a GPU, create() fails only for the missing device;
(ii)  what is not built or invalid is refused: dim != 4, knn_k > 0, an unknown space, a negative max_angle (ZERO_VOLUME), a
      non-finite centre, lvs_fraction 0;
(iii) PrmConfig.space is the field that was `reserved` (offset 196);
(iv)  the Python PRM mirror builds an SO(3) roadmap and refuses a SphereBoxValidityChecker on an SO(3) problem;
(v)   prm_so3.hip compiles for gfx950 without scratch, VGPR spills or flat memory instructions."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest

from oxmpl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oxmpl_amd", "csrc")
FIXTURE = [0.0, 0.0, 0.0, 1.0, math.pi]


@pytest.fixture(scope="module")
def L():
    capi.build_library()
    return capi.lib()


def _no_gpu(L):
    n = C.c_int32()
    return L.oxhip_device_count(C.byref(n)) != capi.OK


def _cfg(**kw):
    cfg = capi.PrmConfig()
    cfg.struct_size, cfg.dim, cfg.space = C.sizeof(capi.PrmConfig), 4, capi.SPACE_SO3
    for i, v in enumerate(kw.pop("bounds", FIXTURE)):
        cfg.bounds[i] = v
    cfg.connection_radius, cfg.lvs_fraction, cfg.max_milestones = 0.5, 0.05, 1000
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _create(L, cfg):
    h = C.c_void_p()
    st = L.oxhip_prm_create(C.byref(cfg), C.byref(h))
    if st == capi.OK:
        L.oxhip_prm_destroy(h)
    return st


def test_space_field_replaces_reserved():
    assert capi.PrmConfig.space.offset == 196 and capi.PrmConfig.space.size == 4
    assert C.sizeof(capi.PrmConfig) == 200


def test_so3_prm_reaches_the_device_check(L):
    if not _no_gpu(L):
        pytest.skip("a GPU is visible here")
    for kw in (dict(), dict(bounds=[0.1, 0.2, 0.3, 0.9, 0.7]), dict(bounds=[0.0, 0.0, 0.0, 1.0, 9.0]),
               dict(bounds=[0.0, 0.0, 0.0, 1.0, float("nan")]), dict(connection_radius=math.inf), dict(connection_radius=0.0),
               dict(connection_radius=2.0), dict(lvs_fraction=0.01), dict(timeout=1.0, max_samples=100)):
        assert _create(L, _cfg(**kw)) == capi.ERR_NO_DEVICE, kw
    with pytest.raises(capi.OxhipError) as ei:
        capi.PRMRoadmap(4, FIXTURE, 0.5, 100, space=capi.SPACE_SO3)
    assert ei.value.status == capi.ERR_NO_DEVICE


@pytest.mark.parametrize("kw,code,msg", [
    (dict(dim=3), capi.ERR_BAD_ARG, b"dim must be 4"),
    (dict(dim=5), capi.ERR_BAD_ARG, b"dim must be 4"),
    (dict(knn_k=8), capi.ERR_BAD_ARG, b"knn_k"),
    (dict(space=1), capi.ERR_BAD_ARG, b"PRM space"),
    (dict(space=3), capi.ERR_BAD_ARG, b"PRM space"),
    (dict(bounds=[0.0, 0.0, 0.0, 1.0, -0.25]), capi.ERR_ZERO_VOLUME, b"max_angle"),
    (dict(bounds=[0.0, 0.0, 0.0, 1.0, -1e-300]), capi.ERR_ZERO_VOLUME, b"max_angle"),
    (dict(bounds=[0.0, math.nan, 0.0, 1.0, 1.0]), capi.ERR_BAD_ARG, b"centre"),
    (dict(bounds=[0.0, 0.0, math.inf, 1.0, 1.0]), capi.ERR_BAD_ARG, b"centre"),
    (dict(bounds=[0.0, 0.0, 1e200, 1.0, 1.0]), capi.ERR_BAD_ARG, b"centre"),
    (dict(lvs_fraction=0.0), capi.ERR_BAD_ARG, b"longest valid segment"),
    (dict(lvs_fraction=1e-9), capi.ERR_BAD_ARG, b"1e6 validity checks"),
    (dict(connection_radius=math.nan), capi.ERR_BAD_ARG, b"NaN"),
])
def test_so3_prm_refuses_what_is_not_built_or_invalid(L, kw, code, msg):
    assert _create(L, _cfg(**kw)) == code, kw
    assert msg in L.oxhip_last_error_string()


def test_real_vector_prm_refuses_an_unknown_space(L):
    """a non-zero `reserved` used to be ignored; the field is now the space kind"""
    cfg = capi.PrmConfig()
    cfg.struct_size, cfg.dim, cfg.space = C.sizeof(capi.PrmConfig), 2, 7
    for i, v in enumerate([0.0, 1.0, 0.0, 1.0]):
        cfg.bounds[i] = v
    cfg.connection_radius, cfg.lvs_fraction, cfg.max_milestones = 0.5, 0.05, 100
    assert _create(L, cfg) == capi.ERR_BAD_ARG


def test_python_prm_mirror_builds_so3_and_refuses_spheres(L):
    from oxmpl_amd.base import ProblemDefinition, SO3ConeValidityChecker, SO3State, SO3StateSpace, SphereBoxValidityChecker
    from oxmpl_amd.geometric import PRM

    class Goal:
        def __init__(self, target, radius):
            self.target, self.radius = target, radius

    s = math.sqrt(0.5)
    pd = ProblemDefinition.from_so3(SO3StateSpace(), SO3State(0.0, s, 0.0, s), Goal(SO3State(0.0, -s, 0.0, s), math.radians(10.0)))
    with pytest.raises(TypeError):
        PRM(5.0, 0.5, pd).setup(SphereBoxValidityChecker())
    with pytest.raises(capi.OxhipError):
        capi.PRMRoadmap(4, [0.0, 0.0, 0.0, 1.0], 0.5, 100, space=capi.SPACE_SO3)   # five values: centre and max_angle
    if _no_gpu(L):
        with pytest.raises(capi.OxhipError) as ei:
            PRM(5.0, 0.5, pd).setup(SO3ConeValidityChecker([(SO3State.identity(), math.radians(44.9))]))
        assert ei.value.status == capi.ERR_NO_DEVICE


def _kernels(asm):
    meta = {}
    for block in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|private_segment_fixed_size|"
                                                        r"group_segment_fixed_size|max_flat_workgroup_size):\s+(\d+)", block)}
    return meta


def test_prm_so3_kernels_have_no_scratch_and_no_flat_loads(tmp_path):
    out = str(tmp_path / "prm_so3.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                           "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "prm_so3.hip")], stderr=subprocess.DEVNULL)
    # the query kernel over SO(3) is prm_kernels.hip's prm_query_kernel<0> (seq_space.hpp): judged here with the file's own
    out_q = str(tmp_path / "prm_kernels.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                           "-S", "--cuda-device-only", "-o", out_q, os.path.join(CSRC, "prm_kernels.hip")], stderr=subprocess.DEVNULL)
    asm = open(out).read() + open(out_q).read()
    meta = {k: v for k, v in _kernels(asm).items() if "prm_so3_" in k or "prm_query_kernelILi0E" in k}
    for part in ("sample_spec", "sample_scan", "sample_compact", "pairs_kernel", "edge_kernelILb1", "edge_kernelILb0", "query_kernelILi0E"):
        assert any(part in k for k in meta), part
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] <= 65536, (name, m)
        body = asm.split(name + ":")[1].split("s_endpgm")[0]
        assert "flat_" not in body and "scratch_" not in body, name
    pairs = [k for k in meta if "pairs_kernel" in k][0]
    body = asm.split(pairs + ":")[1].split("s_endpgm")[0]
    assert "s_load_dwordx8" in body                                      # the i quaternion: one scalar 32-byte load
    assert body.count("v_mul_f64") >= 16 and body.count("v_add_f64") >= 12   # 4 j x (4 mul + 3 add), unfused
