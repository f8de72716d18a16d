#!/usr/bin/env python3
"""Measurement of RRT over SO(3) (rrt_so3.hip): P copies of the reference's SO(3) fixture
(oxmpl/tests/rrt_so3ss_tests.rs: RRT::new(0.5, 0.0), one forbidden cone of 44.9 degrees about the identity, start / goal a quarter
turn either way about y) on distinct ChaCha12 streams, solved to the goal on one MI355X.  Prints one JSON line: problems/s,
iterations/s and the kernel time (HIP events) of the best of a few repeats.  Usage: bench_so3.py [P] [repeats]"""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from oxmpl_amd import capi  # noqa: E402

P = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
REP = int(sys.argv[2]) if len(sys.argv) > 2 else 3


def axis_angle_y(angle):
    return [0.0, math.sin(angle * 0.5), 0.0, math.cos(angle * 0.5)]


start, target = axis_angle_y(math.pi / 2.0), axis_angle_y(-math.pi / 2.0)
g = capi.RRTBatch(4, [0.0, 0.0, 0.0, 1.0, math.pi], 0.5, 0.0, P, 10000, 0.05, True, 42, 0, 0, capi.KERNEL_AUTO, capi.PLANNER_RRT, 0.0,
                  capi.SPACE_SO3)
g.set_spheres([[0.0, 0.0, 0.0, 1.0]], [math.radians(44.9)])
best = None
for rep in range(REP + 1):   # (repeat 0 warms up)
    g.setup(start, target, math.radians(10.0))
    t0 = time.perf_counter()
    st = g.solve(1 << 20)
    wall = time.perf_counter() - t0
    t = g.last_timing()
    c = g.counts()
    if rep and (best is None or t["kernel_ms"] < best["kernel_ms"]):
        best = dict(kernel_ms=t["kernel_ms"], wall_ms=wall * 1e3, launches=t["launches"], solved=int((st == capi.OK).sum()),
                    iterations=int(c["iterations"].sum()), nodes_mean=float(np.mean(c["nodes"])),
                    iterations_max=int(c["iterations"].max()))
best.update(problems=P, problems_per_s=P / (best["kernel_ms"] * 1e-3), iterations_per_s=best["iterations"] / (best["kernel_ms"] * 1e-3))
print(json.dumps(dict(metric="so3_rrt_fixture", **best)))
