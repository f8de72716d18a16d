#!/usr/bin/env python3
"""Measurement of PRM over SO(3) (prm_so3.hip): the reference's SO(3) PRM scene
(oxmpl/tests/prm_so3ss_tests.rs: PRM::new(5.0, 0.5), unbounded space, one forbidden cone of 44.9 degrees about the identity)
built to 16,384 milestones (the Python default) and to 50,000, on one MI355X.  Prints one JSON line: construct wall time (best of
a few repeats), the phase times of last_timing (HIP events), all-pairs rate, in-radius candidates, edges, and for scale the CPU
checker (tests/golden/make_golden_prm_so3.py) on a small roadmap.  Usage: bench_prm_so3.py [repeats]"""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from oxmpl_amd import capi  # noqa: E402
import make_golden_prm_so3 as gp  # noqa: E402
import make_golden_so3 as g3  # noqa: E402

REP = int(sys.argv[1]) if len(sys.argv) > 1 else 3
CONE = ([0.0, 0.0, 0.0, 1.0], math.radians(44.9))
START = g3.quaternion_from_axis_angle([0.0, 1.0, 0.0], math.pi / 2.0)
GOAL = g3.quaternion_from_axis_angle([0.0, 1.0, 0.0], -math.pi / 2.0)


def run(n):
    best = None
    for rep in range(REP + 1):   # (repeat 0 warms up)
        g = capi.PRMRoadmap(4, [0.0, 0.0, 0.0, 1.0, math.pi], 0.5, n, seed=42, space=capi.SPACE_SO3)
        g.set_spheres([CONE[0]], [CONE[1]])
        g.setup(START, GOAL, math.radians(10.0))
        t0 = time.perf_counter()
        g.construct_roadmap()
        wall = time.perf_counter() - t0
        t = g.last_timing()
        _, entries, samples = g.sizes()
        st, path = g.solve()
        q = g.last_timing()["phase_ms"]
        g.close()
        if rep and (best is None or wall < best["construct_ms"] / 1e3):
            pairs = n * (n - 1) / 2
            best = dict(milestones=n, samples=samples, construct_ms=round(wall * 1e3, 3),
                        phase_ms=dict(sample=round(t["phase_ms"][0], 3), pairs=round(t["phase_ms"][1], 3), edges=round(t["phase_ms"][2], 3),
                                      sort_csr=round(t["phase_ms"][3], 3), query=round(q[4], 3), bfs=round(q[5], 3)),
                        pairs_per_s=round(pairs / (t["phase_ms"][1] * 1e-3), 1) if t["phase_ms"][1] > 0 else None,
                        candidates=t["candidates"], edges=entries // 2, solved=st == capi.OK, path_len=len(path))
    return best


out = dict(bench="prm_so3_fixture", gpu=[run(16384), run(50000)])
sc = dict(gp.scenes()["fixture"], max_milestones=300, seed=42)
t0 = time.perf_counter()
gp.prm_construct(None, 0.5, 0.05, g3.Cones(sc["cones"]), 42, 0, 300, 10 ** 9)
out["cpu_checker"] = dict(milestones=300, construct_ms=round((time.perf_counter() - t0) * 1e3, 1))
print(json.dumps(out))
