#!/usr/bin/env python3
"""Measurement of RRT over SO(2) (rrt_so2.hip) on one MI355X, P problems on distinct ChaCha12 streams:
  fixture   the reference's SO(2) fixture (oxmpl/tests/rrt_so2ss_tests.rs; oxmpl_amd.scenarios.so2_band) solved to the goal: about
            52 iterations and 50 nodes per problem, so it measures launch and chain latency
  growth    no arcs, max_distance 0.01, stop_at_goal off, trees grown to 10,000 nodes: the nearest-neighbour scan past the LDS mirror
Per scene: kernel time (HIP events, summed over the launches of a solve), problems/s, iterations/s and microseconds per iteration
of one problem's chain (kernel time over the longest problem's iterations), the best and the median of the timed repeats after one
warm-up repeat.  Prints one JSON line and writes it to profiles/so2/bench_so2.json.  Usage: bench_so2.py [P] [repeats]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from oxmpl_amd import capi, scenarios  # noqa: E402

P = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
REP = int(sys.argv[2]) if len(sys.argv) > 2 else 5


def measure(sc, max_nodes, stop_at_goal, budget):
    g = scenarios.make_so2_batch(sc, P, max_nodes, stop_at_goal, 42)
    runs = []
    for rep in range(REP + 1):   # (repeat 0 warms up: code object load, first allocations)
        g.setup(sc["start"], sc["goal_centre"], sc["goal_radius"])
        t0 = time.perf_counter()
        st = g.solve(budget)
        wall = time.perf_counter() - t0
        t = g.last_timing()
        c = g.counts()
        if rep:
            runs.append(dict(kernel_ms=t["kernel_ms"], wall_ms=wall * 1e3, launches=t["launches"], solved=int((st == capi.OK).sum()),
                             iterations=int(c["iterations"].sum()), iterations_max=int(c["iterations"].max()),
                             nodes_mean=float(np.mean(c["nodes"]))))
    g.close()
    best = dict(min(runs, key=lambda r: r["kernel_ms"]))
    best["kernel_ms_median"] = float(np.median([r["kernel_ms"] for r in runs]))
    best.update(problems=P, repeats=REP, problems_per_s=P / (best["kernel_ms"] * 1e-3),
                iterations_per_s=best["iterations"] / (best["kernel_ms"] * 1e-3),
                us_per_iteration=best["kernel_ms"] * 1e3 / best["iterations_max"])
    return best


fixture = scenarios.so2_band()
growth = dict(fixture, max_distance=0.01, arcs=[], goal_bias=0.05)
out = dict(metric="so2_rrt", fixture=measure(fixture, 10000, True, 1 << 20), growth=measure(growth, 10000, False, 1 << 20))
os.makedirs(os.path.join(ROOT, "profiles", "so2"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "so2", "bench_so2.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
