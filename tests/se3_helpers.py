"""What the SE(3) GPU tests share (tests/test_gpu_se3.py, tests/test_gpu_se3_limits.py): a batch made from a checker scene, and the
bit-for-bit comparison of one of its problems with a checker result (tests/golden/make_golden_se3.py)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_so3 as so3  # noqa: E402
from helpers import bits  # noqa: E402
from oxmpl_amd import capi  # noqa: E402


def config_bounds(sc):
    centre, max_angle = so3.space_bounds(sc["rot_bounds"])
    return [v for pair in sc["bounds_xyz"] for v in pair] + list(centre) + [max_angle]


def make_gpu(sc, n_problems, seed, first_pid, max_nodes=None, debug_flags=0):
    g = capi.RRTBatch(7, config_bounds(sc), sc["max_distance"], sc["goal_bias"], n_problems, max_nodes or sc["max_nodes"], sc["fraction"],
                      True, seed, first_pid, 0, capi.KERNEL_AUTO, capi.PLANNER_RRT_CONNECT, 0.0, capi.SPACE_SE3, debug_flags=debug_flags)
    g.set_body([c for c, _ in sc["body"]], [r for _, r in sc["body"]])
    if sc["obstacles"]:
        g.set_spheres([c for c, _ in sc["obstacles"]], [r for _, r in sc["obstacles"]])
    g.setup(sc["start"], sc["target"], sc["goal_r"])
    return g


def rows(states):
    return np.array(states, dtype=np.float64).reshape(-1, 7)


def assert_same(g, p, res, c=None, gc=None, full=True):
    """res: a checker result (floats) -- counters, end nodes, and with `full` both trees, parents and the merged path"""
    c = c or g.counts()
    gc = gc or g.goal_counts()
    assert [int(c["nodes"][p]), int(gc["nodes"][p])] == list(res["n"]), p
    assert int(c["iterations"][p]) == res["iterations"] and int(c["checksum"][p]) == res["checksum"], p
    assert [int(c["goal_node"][p]), int(gc["end_node"][p])] == list(res["end"]), p
    if not full:
        return
    for w, (gs, gp) in enumerate((g.tree(p), g.goal_tree(p))):
        assert np.array_equal(gp, np.array(res["parents"][w], dtype=np.int32)), (p, w)
        assert np.array_equal(bits(gs), bits(rows(res["states"][w]))), (p, w)
    assert np.array_equal(bits(g.path(p)), bits(rows(res["path"]))), p
