"""Shared by the SO(2) tests (OXHIP_SPACE_SO2, rrt_so2.hip): the CPU checker (tests/golden/make_golden_so2.py), batches built from
its scene dicts, and the bit-for-bit comparison of a problem with a checker run.  kSo2N / kSo2LdsArcs are read from the kernel's
source text, so a limit shape follows the kernel when a constant moves."""
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import make_golden_so2 as so2  # noqa: E402
from helpers import bits, unhex  # noqa: E402

PI = so2.PI


def kernel_constants():
    with open(os.path.join(ROOT, "oxmpl_amd", "csrc", "rrt_so2.hip")) as f:
        src = f.read()
    n = re.search(r"constexpr int kSo2N = (\d+);", src)
    a = re.search(r"constexpr int kSo2LdsArcs = (\d+);", src)
    assert n and a, "rrt_so2.hip no longer declares kSo2N / kSo2LdsArcs as plain constants"
    return int(n.group(1)), int(a.group(1))


K_SO2_N, K_SO2_LDS_ARCS = kernel_constants()


def load_golden():
    with open(os.path.join(ROOT, "tests", "golden", "so2_golden.json")) as f:
        return json.load(f)


def scene_from_params(P):
    return dict(bounds=None if P["bounds"] is None else tuple(unhex(v) for v in P["bounds"]),
                max_distance=unhex(P["max_distance"]), goal_bias=unhex(P["goal_bias"]), fraction=unhex(P["fraction"]),
                start=unhex(P["start"]), target=unhex(P["target"]), goal_r=unhex(P["goal_r"]),
                arcs=[(unhex(lo), unhex(hi)) for lo, hi in P["arcs"]], max_nodes=P["max_nodes"], max_iterations=P["max_iterations"])


def run_from_record(run):
    return dict(run, checksum=int(run["checksum"], 16), states=[unhex(v) for v in run["states"]], path=[unhex(v) for v in run["path"]])


def scene(bounds=None, max_distance=0.2, goal_bias=0.05, fraction=0.05, start=0.0, target=1.0, goal_r=0.1, arcs=(), max_nodes=10000,
          max_iterations=1000):
    return dict(bounds=bounds, max_distance=max_distance, goal_bias=goal_bias, fraction=fraction, start=start, target=target,
                goal_r=goal_r, arcs=list(arcs), max_nodes=max_nodes, max_iterations=max_iterations)


def config_bounds(sc):
    return [-PI, PI] if sc["bounds"] is None else list(sc["bounds"])


def set_arcs(g, arcs):
    g.set_boxes(np.array([lo for lo, _ in arcs], dtype=np.float64).reshape(-1, 1),
                np.array([hi for _, hi in arcs], dtype=np.float64).reshape(-1, 1))


def make_gpu(sc, n_problems, seed, first_pid, max_nodes=None, stop_at_goal=True, kernel=None):
    from oxmpl_amd import capi
    g = capi.RRTBatch(1, config_bounds(sc), sc["max_distance"], sc["goal_bias"], n_problems, max_nodes or sc["max_nodes"],
                      sc["fraction"], stop_at_goal, seed, first_pid, 0, capi.KERNEL_AUTO if kernel is None else kernel,
                      capi.PLANNER_RRT, 0.0, capi.SPACE_SO2)
    set_arcs(g, sc["arcs"])
    g.setup([sc["start"]], [sc["target"]], sc["goal_r"])
    return g


def assert_same(g, p, res, c=None):
    """problem p of batch g equals the checker's run `res`: counts, checksum, goal node, tree, parents and path, bit for bit"""
    c = c or g.counts()
    got = (int(c["nodes"][p]), int(c["iterations"][p]), int(c["accepted"][p]), int(c["checksum"][p]), int(c["goal_node"][p]))
    want = (res["n"], res["iterations"], res["accepted"], res["checksum"], res["goal_node"])
    assert got == want, (p, got, want)
    gs, gp = g.tree(p)
    assert np.array_equal(gp, np.array(res["parents"], dtype=np.int32))
    assert np.array_equal(bits(gs).reshape(-1), bits(np.array(res["states"], dtype=np.float64)))
    assert np.array_equal(bits(g.path(p)).reshape(-1), bits(np.array(res["path"], dtype=np.float64)))


def reference_path_assertions(path, sc):
    """the assertions of test_rrt_finds_path_in_so2ss on a solution path"""
    arcs = so2.Arcs(sc["arcs"])
    assert path and so2.distance(path[0], sc["start"]) < 1e-9
    assert so2.distance(path[-1], sc["target"]) <= sc["goal_r"]
    assert so2.is_so2_path_valid(path, arcs, sc["fraction"])
