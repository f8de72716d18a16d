"""-m gpu: RRT over SO3StateSpace (OXHIP_SPACE_SO3, rrt_so3.hip) against the CPU checker (tests/golden/make_golden_so3.py) and its
golden file, bit for bit: the SO(3) arithmetic (distance, interpolate, ox_acos), trees, parents, counts, checksums and paths --
on the reference's own fixture (oxmpl/tests/rrt_so3ss_tests.rs), on varied scenes, across batch sizes, launch cuts, freeze, warm
starts and a bounded fuzz leg -- and the Python surface on the fixture.  PARITY UNPINNED against oxmpl itself (ox_acos /
ox_sincos are within one ulp of libm, not equal to it)."""
import json
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import make_golden_so3 as so3  # noqa: E402
from helpers import bits, unhex  # noqa: E402
from oxmpl_amd import capi  # noqa: E402


@pytest.fixture(scope="module")
def so3_golden():
    with open(os.path.join(ROOT, "tests", "golden", "so3_golden.json")) as f:
        return json.load(f)


def _bounds(sc):
    centre, max_angle = (None, None) if sc["bounds"] is None else sc["bounds"]
    return [0.0, 0.0, 0.0, 1.0, math.pi] if centre is None else list(centre) + [max_angle]


def make_gpu(sc, n_problems, seed, first_pid, max_nodes=None, debug_flags=0, stop_at_goal=True, kernel=capi.KERNEL_AUTO):
    g = capi.RRTBatch(4, _bounds(sc), sc["max_distance"], sc["goal_bias"], n_problems, max_nodes or sc["max_nodes"], sc["fraction"],
                      stop_at_goal, seed, first_pid, 0, kernel, capi.PLANNER_RRT, 0.0, capi.SPACE_SO3, debug_flags=debug_flags)
    if sc["cones"]:
        g.set_spheres([c for c, _ in sc["cones"]], [r for _, r in sc["cones"]])
    g.setup(sc["start"], sc["target"], sc["goal_r"])
    return g


def assert_same(g, p, res, c=None):
    c = c or g.counts()
    assert int(c["nodes"][p]) == res["n"] and int(c["iterations"][p]) == res["iterations"]
    assert int(c["accepted"][p]) == res["accepted"] and int(c["checksum"][p]) == res["checksum"]
    assert int(c["goal_node"][p]) == res["goal_node"]
    gs, gp = g.tree(p)
    assert np.array_equal(gp, np.array(res["parents"], dtype=np.int32))
    assert np.array_equal(bits(gs), bits(np.array(res["states"], dtype=np.float64).reshape(-1, 4)))
    gpath = g.path(p)
    assert np.array_equal(bits(gpath), bits(np.array(res["path"], dtype=np.float64).reshape(-1, 4)))


def _scene_from_params(P):
    hx = lambda row: [unhex(v) for v in row]  # noqa: E731
    return dict(bounds=None if P["bounds"] is None else (hx(P["bounds"][0]), unhex(P["bounds"][1])),
                max_distance=unhex(P["max_distance"]), goal_bias=unhex(P["goal_bias"]), fraction=unhex(P["fraction"]),
                start=hx(P["start"]), target=hx(P["target"]), goal_r=unhex(P["goal_r"]),
                cones=[(hx(c), unhex(r)) for c, r in P["cones"]], max_nodes=P["max_nodes"], max_iterations=P["max_iterations"])


def _unit(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _pairs_at(rng, n, cosines):
    """pairs (a, b) of unit quaternions with dot(a, b) ~ the given cosines (b = cos a + sin u, u orthogonal to a)"""
    a = _unit(rng, n)
    u = rng.normal(size=(n, 4))
    u -= (u * a).sum(axis=1, keepdims=True) * a
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    c = np.asarray(cosines, dtype=np.float64)
    b = c[:, None] * a + np.sqrt(np.maximum(0.0, 1.0 - c * c))[:, None] * u
    return a, b


def test_device_arithmetic_equals_the_restatement():
    rng = np.random.default_rng(3)
    n_rand = 60000
    a, b = _unit(rng, n_rand), _unit(rng, n_rand)
    edges = []
    for c0 in (0.9995, 1.0 - 1e-9, 1.0):
        c = c0 + rng.integers(-40, 41, size=2000) * 2.0 ** -52
        ea, eb = _pairs_at(rng, 2000, np.minimum(c, 1.0))
        edges += [(ea, eb), (ea, -eb)]   # and the sign flip
    anti = _unit(rng, 500)
    edges += [(anti, -anti), (anti, anti)]   # antipodal pairs (one rotation) and equal pairs
    A = np.concatenate([a] + [e[0] for e in edges])
    B = np.concatenate([b] + [e[1] for e in edges])
    t = rng.random(A.shape[0])
    t[::7] = 0.0
    t[3::7] = 1.0
    d_gpu = capi.so3_op_batch(0, A, B)
    want_d = np.array([so3.distance(x, y) for x, y in zip(A.tolist(), B.tolist())])
    assert np.array_equal(bits(d_gpu), bits(want_d))
    i_gpu = capi.so3_op_batch(1, A, B, t)
    want_i = np.array([so3.interpolate(x, y, tt) for x, y, tt in zip(A.tolist(), B.tolist(), t.tolist())])
    assert np.array_equal(bits(i_gpu), bits(want_i))
    x = np.concatenate([rng.random(40000), np.abs((A * B).sum(axis=1))[:20000], [0.0, 0.5, 1.0, 1e-300, 2.0 ** -57, 0.9995, 1.0 - 1e-9],
                        np.nextafter(1.0 - 1e-9, np.arange(-3, 4) * 1.0), -rng.random(2000), [1.5, -1.5, np.nan]])
    a_gpu = capi.so3_op_batch(2, x)
    want_a = np.array([so3.ox_acos(v) for v in x.tolist()])
    assert np.array_equal(bits(a_gpu), bits(want_a))


@pytest.mark.parametrize("scene", ["fixture", "bounded", "bias1", "tiny"])
def test_golden_cases_match_exactly(so3_golden, scene):
    sc = _scene_from_params(so3_golden[scene]["params"])
    for run in so3_golden[scene]["runs"]:
        g = make_gpu(sc, 1, run["seed"], run["pid"])
        st = g.solve(sc["max_iterations"])
        assert (st[0] == capi.OK) == (run["goal_node"] >= 0)
        res = dict(run, checksum=int(run["checksum"], 16), states=[[unhex(v) for v in r] for r in run["states"]],
                   path=[[unhex(v) for v in r] for r in run["path"]])
        assert_same(g, 0, res)
        g.close()


def test_1024_fixture_problems():
    sc = so3.fixture_scene()
    cones = so3.Cones(sc["cones"])
    P, seed, pid0 = 1024, 42, 1000
    g = make_gpu(sc, P, seed, pid0)
    st = g.solve(200000)
    assert (st == capi.OK).all()
    c = g.counts()
    for p in range(32):
        assert_same(g, p, so3.run_scene(sc, seed, pid0 + p, max_iterations=200000), c)
    for p in range(P):   # the reference's assertions (rrt_so3ss_tests.rs:190-213) on every problem
        path = g.path(p).tolist()
        assert path and so3.distance(path[0], sc["start"]) < 1e-9
        assert so3.distance(path[-1], sc["target"]) <= sc["goal_r"]
        assert so3.is_so3_path_valid(path, cones, sc["fraction"]), p
    # problem 0 does not depend on the batch size or on how the budget is cut into solve calls
    for cut in (None, 1, 7, 64):
        g1 = make_gpu(sc, 1 if cut is None else 3, seed, pid0)
        if cut is None:
            g1.solve(200000)
        else:
            for _ in range(200000 // cut):
                if (g1.solve(cut)[0] == capi.OK):
                    break
        c1 = g1.counts()
        for k in ("nodes", "iterations", "accepted", "checksum", "goal_node"):
            assert c1[k][0] == c[k][0], (cut, k)
        assert np.array_equal(bits(g1.tree(0)[0]), bits(g.tree(0)[0])) and np.array_equal(bits(g1.path(0)), bits(g.path(0)))
        g1.close()
    g.close()


def test_freeze_and_warm_start_match_the_checker():
    sc = so3.fixture_scene()
    # freeze: steady iterations against the one-node tree
    g = make_gpu(sc, 2, 5, 20)
    g.solve(700, freeze=True)
    c = g.counts()
    for p in range(2):
        assert_same(g, p, so3.run_scene(sc, 5, 20 + p, max_iterations=700, freeze=True), c)
    g.close()
    # warm start: a planted tree larger than the LDS mirror (nodes beyond 1,024 come from HBM), grown and frozen
    rng = np.random.default_rng(9)
    cones = so3.Cones(sc["cones"])
    nodes = [sc["start"]]
    while len(nodes) < 1500:
        q = _unit(rng, 1)[0].tolist()
        if cones.is_valid(q):
            nodes.append(q)
    parents = [-1] + [int(rng.integers(0, i)) for i in range(1, 1500)]
    for freeze, iters in ((False, 150), (True, 150)):
        g = make_gpu(sc, 2, 11, 40, max_nodes=4000)
        for p in range(2):
            g.set_tree(p, np.array(nodes), np.array(parents))
        g.solve(iters, freeze=freeze)
        c = g.counts()
        for p in range(2):
            res = so3.rrt_solve(None, sc["max_distance"], sc["goal_bias"], sc["fraction"], cones, sc["start"], sc["target"], sc["goal_r"],
                                11, 40 + p, iters, 4000, freeze=freeze, tree=nodes, parents=parents)
            assert_same(g, p, res, c)
        g.close()


def test_fuzz_against_the_checker():
    rng = np.random.default_rng(20261015)
    for case in range(30):
        centre = _unit(rng, 1)[0].tolist()
        max_angle = float(rng.choice([0.0, 0.3, 0.8, 1.3, math.pi, 5.0]))
        n_cones = int(rng.choice([0, 1, 3, 8, 40]))   # (40: the cone table is read from HBM)
        cones = [(_unit(rng, 1)[0].tolist(), float(rng.uniform(0.02, 0.3))) for _ in range(n_cones)]
        start = centre if rng.random() < 0.5 else _unit(rng, 1)[0].tolist()
        sc = dict(bounds=(centre, max_angle), max_distance=float(rng.choice([0.005, 0.05, 0.3, 1.0, 2.0])),
                  goal_bias=float(rng.choice([0.0, 0.05, 0.3, 1.0])), fraction=float(rng.choice([0.05, 0.1, 0.5])),
                  start=start, target=_unit(rng, 1)[0].tolist(), goal_r=float(rng.uniform(0.05, 0.4)), cones=cones,
                  max_nodes=int(rng.choice([40, 400])), max_iterations=120)
        seed, pid = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 1000))
        flags = capi.DEBUG_SO3_SERIAL_SAMPLER if case % 4 == 3 else 0
        stop = bool(case % 5 != 4)
        g = make_gpu(sc, 2, seed, pid, debug_flags=flags, stop_at_goal=stop, kernel=capi.KERNEL_STREAM if case % 2 else capi.KERNEL_AUTO)
        cut = int(rng.choice([1, 7, 64, 120]))
        done = 0
        while done < sc["max_iterations"]:
            step = min(cut, sc["max_iterations"] - done)
            g.solve(step)
            done += step
        c = g.counts()
        for p in range(2):
            res = so3.run_scene(sc, seed, pid + p, stop_at_goal=stop)
            assert_same(g, p, res, c)
        g.close()


def test_is_valid_and_check_motion_answer_in_so3():
    sc = so3.scenes()["bounded"]
    g = make_gpu(sc, 1, 0, 0)
    cones = so3.Cones(sc["cones"])
    rng = np.random.default_rng(4)
    qs = np.concatenate([_unit(rng, 3000), np.array([c for c, _ in sc["cones"]])])
    assert np.array_equal(g.is_valid(qs), np.array([cones.is_valid(q) for q in qs.tolist()]))
    a, b = _unit(rng, 500), _unit(rng, 500)
    want = np.array([so3.check_motion(cones, sc["fraction"], x, y) for x, y in zip(a.tolist(), b.tolist())])
    assert np.array_equal(g.check_motion(a, b), want)
    assert not want.all() and want.any()
    with pytest.raises(capi.OxhipError) as ei:
        g.set_boxes(np.zeros((1, 4)), np.ones((1, 4)))
    assert ei.value.status == capi.ERR_BAD_ARG
    g.close()


def test_python_surface_solves_the_reference_fixture():
    from oxmpl_amd.base import ProblemDefinition, SO3ConeValidityChecker, SO3State, SO3StateSpace
    from oxmpl_amd.geometric import RRT

    class SO3GoalRegion:
        def __init__(self, space, target, radius):
            self.space, self.target, self.radius = space, target, radius

        def is_satisfied(self, state):
            return self.space.distance(state, self.target) <= self.radius

    sc = so3.fixture_scene()
    space = SO3StateSpace()
    start, target = SO3State(*sc["start"]), SO3State(*sc["target"])
    goal = SO3GoalRegion(space, target, math.radians(10.0))
    pd = ProblemDefinition.from_so3(space, start, goal)
    checker = SO3ConeValidityChecker([(SO3State.identity(), math.radians(44.9))])
    planner = RRT(0.5, 0.0, pd)
    planner.setup(checker)
    path = planner.solve(5.0)
    states = path.states
    assert states and all(isinstance(s, SO3State) for s in states)
    assert space.distance(states[0], start) < 1e-9
    assert goal.is_satisfied(states[-1])
    assert so3.is_so3_path_valid([s.values for s in states], so3.Cones(sc["cones"]), sc["fraction"])
    assert all(planner.is_state_valid(s) for s in states)
