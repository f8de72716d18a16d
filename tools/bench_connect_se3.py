#!/usr/bin/env python3
"""Measurement of RRTConnect over SE(3): P independent problems of the field scene (a rod of five spheres
among 64 random spheres) solved to completion on one MI355X -- best of 3 after a warm-up, HIP-event kernel time -- the slot scene
next to it, and the per-iteration latency by the slope method of tools/probe_connect_slope.py (kernel time of a batch cut after
8 .. 64 iterations; no problem of either scene finishes in fewer than 10).  One JSON line, also written under profiles/.
Usage: bench_connect_se3.py [problems] [output.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from oxmpl_amd import capi, scenarios  # noqa: E402

P = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "se3_connect", "bench_connect_se3.json")
BUDGET = 20000


def completion(sc, n):
    """kernel ms of n problems solved to completion: a warm-up, then three runs (the same problems: seed 42, streams 0 .. n - 1)"""
    ms = []
    for rep in range(4):
        g = scenarios.make_se3_batch(sc, n, 10000, 42)
        st = g.solve(BUDGET)
        assert (st == capi.OK).all()
        if rep:
            ms.append(g.last_timing()["kernel_ms"])
        c, gc = g.counts(), g.goal_counts()
        g.close()
    its = c["iterations"]
    return dict(problems=n, kernel_ms_best=min(ms), kernel_ms_runs=ms, spread=(max(ms) - min(ms)) / min(ms),
                problems_per_s=n / (min(ms) * 1e-3), iterations=int(its.sum()), iterations_max=int(its.max()),
                iterations_median=float(np.median(its)), iterations_per_s=float(its.sum()) / (min(ms) * 1e-3),
                mean_nodes_both_trees=float((c["nodes"] + gc["nodes"]).mean()))


def slope(sc, n):
    """kernel ms against the iteration budget of one launch; the slope between 8 and 32 is the latency of one iteration of the
    slowest wave (every problem is still running at 8 iterations; later cuts lose the problems that finished, see still_running)"""
    rows = {}
    for budget in (8, 16, 32, 64):
        ts = []
        for rep in range(3):
            g = scenarios.make_se3_batch(sc, n, 10000, 42)
            g.solve(budget)
            ts.append(g.last_timing()["kernel_ms"])
            running = int((g.counts()["stop_reason"] == capi.STOP_ITERATIONS).sum())
            g.close()
        rows[budget] = dict(kernel_ms=min(ts), still_running=running)
    return dict(problems=n, cuts=rows, us_per_iteration=(rows[32]["kernel_ms"] - rows[8]["kernel_ms"]) / 24.0 * 1e3)


def sweep_pair(sc, n):
    """the motion check's obstacle sweep, the first working kernel's (OXHIP_DEBUG_SE3_BRANCHY_SWEEP) against the product's, same
    problems, alternating within this process: a warm-up round, then three timed rounds of each"""
    ms = {"first_kernel_sweep": [], "product": []}
    for rep in range(4):
        for name, flag in (("first_kernel_sweep", capi.DEBUG_SE3_BRANCHY_SWEEP), ("product", 0)):
            g = scenarios.make_se3_batch(sc, n, 10000, 42, debug_flags=flag)
            assert (g.solve(BUDGET) == capi.OK).all()
            if rep:
                ms[name].append(g.last_timing()["kernel_ms"])
            g.close()
    return dict(problems=n, kernel_ms=ms, best={k: min(v) for k, v in ms.items()},
                ratio_best=min(ms["first_kernel_sweep"]) / min(ms["product"]))


def stamps(sc):
    """where the cycles of problem 0's iterations go: the diagnostic instantiation (enable_stamps), one problem alone"""
    g = scenarios.make_se3_batch(sc, 1, 10000, 42)
    g.enable_stamps()
    g.solve(BUDGET)
    w = [int(v) for v in g.stamps()[:7]]
    chk = int(g.counts()["checksum"][0])
    g.close()
    h = scenarios.make_se3_batch(sc, 1, 10000, 42)
    h.solve(BUDGET)
    assert int(h.counts()["checksum"][0]) == chk   # the stamped build computes what the product does
    h.close()
    its = max(w[5], 1)
    names = ("sample", "nearest", "steer", "motion_check")
    out = {n: w[k] / its for k, n in enumerate(names)}
    out.update(other=(w[4] - sum(w[:4])) / its, total=w[4] / its, iterations=w[5], extends=w[6])
    return out   # cycles per iteration


field, slot = scenarios.se3_field(), scenarios.se3_slot()
res = {"planner": "RRTConnect/SE(3)", "workload": "SE(3), rod of 5 spheres, field of 64 spheres, %d problems to completion" % P,
       "field": completion(field, P), "slot": completion(slot, min(P, 256)),
       "slope_field": [slope(field, 1), slope(field, P)], "slope_slot": [slope(slot, 1), slope(slot, min(P, 256))],
       "sweep_before_after": {"field": sweep_pair(field, P), "slot": sweep_pair(slot, min(P, 256))},
       "cycles_per_iteration_problem_0": {"field": stamps(field), "slot": stamps(slot)}}
res["kernel_ms"] = res["field"]["kernel_ms_best"]
res["problems_per_s"] = res["field"]["problems_per_s"]
line = json.dumps(res)
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    f.write(line + "\n")
print(line)
