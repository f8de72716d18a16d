"""CPU: prm_bfs_path (oxhip_host.hpp), the graph search and path reconstruction of oxhip_prm_solve, on hand-made roadmaps
(tests/cpp/test_prm_bfs.cpp).  A stand-alone program with its own main, built with AddressSanitizer and UBSan; it touches no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prm_bfs_path_on_hand_made_roadmaps(tmp_path):
    exe = str(tmp_path / "test_prm_bfs")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "test_prm_bfs.cpp"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    assert "prm_bfs_path: all cases passed" in r.stdout and "FAILED" not in r.stdout
