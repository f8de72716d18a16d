"""-m gpu: rrt_so3.hip at the seams its other tests leave unpinned: a tree that grows across the edge of the LDS mirror inside a
launch, the node cap, cone counts around the staged table's size with the last cone deciding, and check_motion rows around the
64-state pass.  The oracle is the CPU checker (tests/golden/make_golden_so3.py: rrt_solve, check_motion), bit for bit."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_so3 import _unit, assert_same, make_gpu, so3  # noqa: E402

K_MIRROR, K_LDS_CONES = 1024, 32   # kSo3N, kSo3LdsCones of rrt_so3.hip
PLANTED = 1000


@pytest.fixture(scope="module")
def planted():
    """the fixture's space without cones (every state is valid, so every iteration inserts) and a tree of 1,000 nodes"""
    sc = dict(so3.fixture_scene(), cones=[], goal_bias=0.05)
    rng = np.random.default_rng(31)
    nodes = [sc["start"]] + _unit(rng, PLANTED - 1).tolist()
    parents = [-1] + [int(rng.integers(0, i)) for i in range(1, PLANTED)]
    return sc, nodes, parents


def _solve_planted(planted, seed, pid, iterations, max_nodes, **kw):
    sc, nodes, parents = planted
    return so3.rrt_solve(None, sc["max_distance"], sc["goal_bias"], sc["fraction"], so3.Cones(), sc["start"], sc["target"], sc["goal_r"],
                         seed, pid, iterations, max_nodes, tree=nodes, parents=parents, **kw)


def test_a_tree_grows_across_the_mirror_edge_inside_a_launch(planted):
    """1,000 planted nodes, 40 insertions per launch: node 1,024 is stored inside the first launch (the nearest search then reads
    the mirror and HBM), and the second launch starts beyond the mirror"""
    sc, nodes, parents = planted
    g = make_gpu(sc, 2, 17, 60, max_nodes=1100, stop_at_goal=False)
    for p in range(2):
        g.set_tree(p, np.array(nodes), np.array(parents))
    for done in (40, 80):
        g.solve(40)
        c = g.counts()
        for p in range(2):
            res = _solve_planted(planted, 17, 60 + p, done, 1100, stop_at_goal=False)
            assert res["n"] == PLANTED + done and (done == 80 or PLANTED < K_MIRROR < res["n"])
            assert_same(g, p, res, c)
    g.close()


def test_the_node_cap_leaves_the_stream_where_the_loop_does(planted):
    """the tree fills at iteration 30 of a launch of 100; the stream position the stop leaves is not readable, so a frozen launch
    (which ignores the node cap) continues from it: its checksum folds in the samples drawn from that position on"""
    sc, nodes, parents = planted
    first = _solve_planted(planted, 23, 7, 100, 1030, stop_at_goal=False)
    assert first["n"] == 1030 and first["iterations"] == 30
    g = make_gpu(sc, 1, 23, 7, max_nodes=1030, stop_at_goal=False)
    g.set_tree(0, np.array(nodes), np.array(parents))
    g.solve(100)
    assert_same(g, 0, first)
    assert int(g.counts()["stop_reason"][0]) == 2
    g.solve(50)   # full: nothing runs
    assert_same(g, 0, first)
    assert int(g.counts()["stop_reason"][0]) == 2
    g.solve(30, freeze=True)
    frozen = so3.rrt_solve(None, sc["max_distance"], sc["goal_bias"], sc["fraction"], so3.Cones(), sc["start"], sc["target"], sc["goal_r"],
                           23, 7, 30, 1030, stop_at_goal=False, freeze=True, tree=first["states"], parents=first["parents"],
                           draws=first["rng_draws"])
    Pm = pow(so3.mg.FNV_P, 30, 1 << 64)
    want = (first["checksum"] * Pm + frozen["checksum"] - so3.mg.FNV_BASIS * Pm) & so3.M64
    c = g.counts()
    assert int(c["iterations"][0]) == first["iterations"] + 30 and int(c["checksum"][0]) == want and int(c["nodes"][0]) == first["n"]
    assert int(c["accepted"][0]) == first["accepted"] + frozen["accepted"]
    g.close()


def _scene_with_a_deciding_last_cone(count):
    """the fixture's cone, small cones up to count - 1, and a last one on a node the planner inserts without it: with it that
    motion is refused.  Returns the scene and the checker's run of it."""
    rng = np.random.default_rng(count)
    cones = so3.fixture_scene()["cones"] + [(q, 0.03) for q in _unit(rng, count - 2).tolist()]
    sc = dict(so3.fixture_scene(), cones=cones, fraction=0.5, max_nodes=400, max_iterations=100)   # (fraction 0.5: 7 states per motion)
    without = so3.run_scene(sc, 3, count, stop_at_goal=False)
    assert without["n"] > 8
    sc = dict(sc, cones=cones + [(without["states"][without["n"] // 2], 0.02)])
    assert len(sc["cones"]) == count
    with_last = so3.run_scene(sc, 3, count, stop_at_goal=False)
    assert (with_last["n"], with_last["checksum"]) != (without["n"], without["checksum"])   # the last cone decides
    return sc, with_last


@pytest.mark.parametrize("count", [K_LDS_CONES, K_LDS_CONES + 1])
def test_cone_counts_around_the_staged_table(count):
    """32 cones fill the staged table, 33 are read from HBM; the last cone of either decides a motion"""
    sc, want = _scene_with_a_deciding_last_cone(count)
    g = make_gpu(sc, 1, 3, count, stop_at_goal=False)
    g.solve(100)
    assert_same(g, 0, want)
    g.close()


def _motion_rows():
    """rows (from, to, states, index of the one invalid state or None) and the cones that make them so: every row lies on a great
    circle of its own, a row with an invalid state has a cone of radius 1e-3 on that state (the states lie 0.011 apart)"""
    fraction = 0.07
    res = so3.lvsl(fraction) * 0.1
    rng = np.random.default_rng(64)
    rows, cones = [], []
    for states, bad_at in ((63, [62]), (64, [63]), (65, [63, 64]), (128, [63, 64, 127]), (129, [63, 64, 127, 128])):
        for bad in bad_at + [None] * len(bad_at):   # (and the all-valid twin of each)
            a = _unit(rng, 1)[0]
            u = rng.normal(size=4)
            u -= (u * a).sum() * a
            u /= np.linalg.norm(u)
            d = (states - 0.5) * res
            a, b = a.tolist(), (math.cos(d) * a + math.sin(d) * u).tolist()
            assert so3.mg.num_steps(so3.distance(a, b), so3.lvsl(fraction)) == states
            if bad is not None:
                cones.append((so3.interpolate(a, b, float(bad + 1) / float(states)), 1e-3))
            rows.append((a, b, states, bad))
    return fraction, rows, cones


def test_check_motion_rows_around_the_64_state_pass():
    """motions of 63, 64, 65, 128 and 129 states whose one invalid state is the last of a pass or the first of the next, and
    their all-valid twins"""
    fraction, rows, cones = _motion_rows()
    checker = so3.Cones(cones)
    for a, b, states, bad in rows:   # the rows are what they are meant to be
        invalid = [s for s in range(states) if not checker.is_valid(so3.interpolate(a, b, float(s + 1) / float(states)))]
        assert invalid == ([] if bad is None else [bad]), (states, bad, invalid)
    want = [so3.check_motion(checker, fraction, a, b) for a, b, _, _ in rows]
    assert want == [bad is None for _, _, _, bad in rows]
    g = make_gpu(dict(so3.fixture_scene(), cones=cones, fraction=fraction), 1, 0, 0)
    got = g.check_motion(np.array([r[0] for r in rows]), np.array([r[1] for r in rows])).astype(bool).tolist()
    assert got == want
    g.close()
