"""The C++ host mirror's PRM::simplify_batch / is_valid / check_motion (include/oxmpl/oxmpl.hpp) compiled against the C ABI.  CPU: it
must build, link and refuse to plan without a GPU (exit 77).  GPU: simplified paths keep their ends, pass check_motion link by
link and are no longer; a refused solve_batch leaves what simplify_batch answers for as it was (exit 0)."""
import os
import subprocess

import pytest

from oxmpl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, name="test_prm_simplify_rvss"):
    capi.build_library()
    exe = str(tmp_path / name)
    libdir = os.path.join(ROOT, "oxmpl_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe,
                           "-L", libdir, "-loxmpl_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_prm_simplify_builds_and_refuses_without_gpu(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode in (0, 77), r.stdout + r.stderr
    if r.returncode == 77:
        assert "refused as designed" in r.stdout


@pytest.mark.gpu
def test_cpp_prm_simplify_on_the_wall_scene(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PRM simplify batch test passed!" in r.stdout
