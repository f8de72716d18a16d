"""-m gpu: bench.py at N = 1, small shape (64 problems, 512 iterations per step), once plain and once with --full.
A plain run prints the headline line only; --full adds the oracle checks and the secondary rows, each of which refuses the line
unless the GPU agrees with the oracle or with the main run."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, ITERS, STEPS, WARMUP = 64, 512, 2, 1
FULL_ONLY = ("cpu_baseline", "secondary", "secondary_lanes", "secondary_f64", "secondary_rrt_star", "secondary_rrt_connect",
             "hbm_copy_peak_GBps")


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
           "--problems", str(P), "--iters", str(ITERS)] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 1 and out["steps"] == STEPS and out["warmup"] == WARMUP
    assert out["unit"] == "iterations/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["value"] > 0 and abs(out["value"] - P * ITERS / (out["ms_per_step"] * 1e-3)) / out["value"] < 1e-6
    assert out["roofline"]["achieved"] > 0
    return out


def test_bench_py_plain_run_is_headline_only():
    out = _bench()
    assert out["full"] is False
    for key in FULL_ONLY:
        assert key not in out, key
    assert out["roofline"].get("hbm_copy_peak_GBps") is None


def test_bench_py_full_run_checks_against_oracle_and_secondary_kernels():
    out = _bench("--full")
    assert out["full"] is True
    assert out["cpu_baseline"]["value"] > 0 and out["cpu_baseline"]["threads"] >= 1
    assert out["hbm_copy_peak_GBps"] > 0
    kname = out["config"]["kernel"]
    for key, kind in (("secondary", "stream"), ("secondary_lanes", "lanes"), ("secondary_f64", "resident")):
        if kname != kind and key in out:
            assert out[key]["checksums_equal_main_run"] is True, key
    assert out["secondary_rrt_star"]["problem0_parents_costs_checksum_equal_oracle"] is True
    rows = out["secondary_rrt_connect"]
    assert set(rows) == {"se2_256_segments", "r3_64_spheres"}
    assert all(row["two_problems_equal_oracle"] is True for row in rows.values())
