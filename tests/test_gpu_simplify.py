"""-m gpu: the whole batch's paths, extracted and shortcut on the device (path_simplify.hip).

Yardsticks, all of them existing entry points or CPU code: RRTBatch.path(p) for the extraction (bit for bit),
RRTBatch.check_motion for every bit of the pair matrix, the Python DP of tests/simplify_helpers.py over those verdicts and over
distance_batch / so3_op_batch for whole results, and tests/golden/simplify_golden.json (the CPU oracle's own paths, verdicts and
distances) for the scenes that have an oracle check_motion.

Every path here comes from a solve.  A path of any other shape can be planted: set_tree, then revalidate_trees() while the batch has
no obstacles (nothing is removed, goal_node becomes the lowest index >= 1 whose state satisfies the goal), then the obstacles;
tests/test_gpu_simplify_limits.py does that for long, tying, far-away and degenerate paths.  L = 1 alone cannot be produced through the
ABI, since goal_node is never the root: the shortest path a batch can hold has two states (the kernels take L = 1 as the model does;
tests/test_simplify_dp_model.py covers it there)."""
import json
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_so3 as so3  # noqa: E402

from oxmpl_amd import capi, scenarios  # noqa: E402
from helpers import bits, unhex  # noqa: E402
import simplify_helpers as sh  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = sh.SEED


# ------------------------------------------------------------------------------------------------ batches (built once)

def _so3_batch(P, sc=None, first_pid=0):
    sc = sc or so3.fixture_scene()
    bounds = [0.0, 0.0, 0.0, 1.0, math.pi] if sc["bounds"] is None else list(sc["bounds"][0]) + [sc["bounds"][1]]
    g = capi.RRTBatch(4, bounds, sc["max_distance"], sc["goal_bias"], P, sc["max_nodes"], sc["fraction"], True, SEED, first_pid, 0,
                      capi.KERNEL_AUTO, capi.PLANNER_RRT, 0.0, capi.SPACE_SO3)
    g.set_spheres([c for c, _ in sc["cones"]], [r for _, r in sc["cones"]])
    g.setup(sc["start"], sc["target"], sc["goal_r"])
    g.solve(sc["max_iterations"])
    return g


def _r6_scene():
    start, goal = [1.0] * 6, [9.0] * 6
    return dict(dim=6, bounds=[(0.0, 10.0)] * 6, max_distance=1.0, goal_bias=0.05, lvs_fraction=0.05, start=start, goal_centre=goal,
                goal_radius=1.5, boxes=None,
                spheres=scenarios.sphere_field(seed=0x5EED0005, n=32, dim=6, lo=1.0, hi=9.0, rmin=2.0, rmax=3.5, keep_clear=[start, goal]))


_BUILDERS = {
    "config1": lambda: _solved(scenarios.make_batch(scenarios.config1(), 64, 10000, True, SEED)),
    "config2": lambda: _solved(scenarios.make_batch(scenarios.config2(), 8, 10000, True, SEED)),
    "wall": lambda: _solved(scenarios.make_batch(scenarios.wall(), 8, 10000, True, SEED)),
    "connect": lambda: _solved(scenarios.make_batch(scenarios.config2(), 64, 10000, True, SEED, planner=capi.PLANNER_RRT_CONNECT)),
    "star": lambda: _solved(scenarios.make_batch(scenarios.config1(), 64, 4000, False, SEED, planner=capi.PLANNER_RRT_STAR,
                                                 search_radius=1.0), sh.STAR_ITERATIONS, need_all=False),
    "se2": lambda: _solved(scenarios.make_se2_batch(scenarios.config4(), 16, 10000, SEED), 10 ** 6),
    "so3": lambda: _so3_batch(16),
    "so3_bounded": lambda: _so3_batch(16, so3.scenes()["bounded"]),   # three cones inside a bounded cone of freedom
    "se3": lambda: _solved(scenarios.make_se3_batch(scenarios.se3_field(), 16, 10000, SEED), 20000),
    "r6": lambda: _solved(scenarios.make_batch(_r6_scene(), 4, 10000, True, SEED)),
    "free": lambda: _solved(scenarios.make_batch(dict(scenarios.config1(), spheres=None), 4, 10000, True, SEED)),
}
_CACHE = {}


def _solved(g, budget=sh.BUDGET, need_all=True):
    st = g.solve(budget)
    assert not need_all or (st == capi.OK).all()
    return g


def batch(name):
    if name not in _CACHE:
        _CACHE[name] = _BUILDERS[name]()
    return _CACHE[name]


def _split(offsets, rows):
    return [rows[int(offsets[p]):int(offsets[p + 1])] for p in range(len(offsets) - 1)]


def _distance(g, a, b):
    if g.space == capi.SPACE_SO3:
        return capi.so3_op_batch(0, a, b)
    return capi.distance_batch(a, b)


def _model(g, path, max_span=0):
    """the Python DP over the entry points' own verdicts and distances"""
    L = len(path)
    if L < 2:
        return sh.shortcut_dp(L, None, None, max_span)
    ii, jj = np.triu_indices(L, 1)
    keep = (jj - ii) <= sh.span_of(L, max_span)
    ii, jj = ii[keep], jj[keep]
    d = dict(zip(zip(ii.tolist(), jj.tolist()), _distance(g, path[ii], path[jj]).tolist()))
    v = dict(zip(zip(ii.tolist(), jj.tolist()), g.check_motion(path[ii], path[jj]).tolist()))
    return sh.shortcut_dp(L, lambda i, j: v[(i, j)], lambda i, j: d[(i, j)], max_span)


def _results(g, max_span=0, chunk=0):
    g.simplify_paths(max_span, chunk)
    off, rows, idx, raw, simp, checks = g.simplified_paths()
    return dict(off=off, rows=rows, idx=idx, raw=raw, simp=simp, checks=checks)


def _assert_equals_model(g, problems, max_span=0):
    roff, rrows = g.paths()
    raw_paths = _split(roff, rrows)
    r = _results(g, max_span)
    for p in problems:
        idx, raw, cost, checks = _model(g, raw_paths[p], max_span)
        a, b = int(r["off"][p]), int(r["off"][p + 1])
        assert r["idx"][a:b].tolist() == idx, p
        assert bits(r["raw"][p]) == bits(raw) and bits(r["simp"][p]) == bits(cost), p
        assert int(r["checks"][p]) == checks == sh.expected_checks(len(raw_paths[p]), max_span)
        assert np.array_equal(bits(r["rows"][a:b]), bits(raw_paths[p][idx]))


# ------------------------------------------------------------------------------------------------ extraction

@pytest.mark.parametrize("name", ["config1", "connect", "star", "se2", "so3", "se3"])
def test_paths_equal_the_loop_of_get_path_bit_for_bit(name):
    g = batch(name)
    g.extract_paths()
    off, rows = g.paths()
    assert off[0] == 0 and int(off[-1]) == len(rows) and rows.shape[1] == g.dim
    n_solved = 0
    for p in range(g.n_problems):
        ref = g.path(p)
        got = rows[int(off[p]):int(off[p + 1])]
        assert got.shape == ref.shape and np.array_equal(bits(got), bits(ref)), (name, p)
        n_solved += len(ref) > 0
    assert n_solved >= g.n_problems // 2
    if name == "connect":   # the splice: some solutions end in the goal tree, and the goal-tree part is more than its root
        assert (g.goal_counts()["end_node"] >= 0).any()


def test_a_batch_of_one_and_a_batch_with_unsolved_problems():
    sc = scenarios.config1()
    g1 = _solved(scenarios.make_batch(sc, 1, 10000, True, SEED, first_problem_id=5))
    g1.extract_paths()
    off, rows = g1.paths()
    assert np.array_equal(bits(rows), bits(g1.path(0))) and off.tolist() == [0, len(rows)]
    g1.close()
    # an iteration budget that the oracle's counts show about half the problems exceed
    P = 16
    planners = [sh.oracle_rrt(sc, p) for p in range(P)]
    for o in planners:
        o.solve(sh.BUDGET)
    budget = int(np.median([o.iterations for o in planners]))
    g = scenarios.make_batch(sc, P, 10000, True, SEED)
    st = g.solve(budget)
    assert (st == capi.OK).any() and (st != capi.OK).any()
    g.extract_paths()
    off, rows = g.paths()
    for p in range(P):
        ref = g.path(p)
        assert (len(ref) > 0) == (st[p] == capi.OK)
        assert np.array_equal(bits(rows[int(off[p]):int(off[p + 1])]), bits(ref))
        if st[p] == capi.OK:
            assert np.array_equal(bits(ref), bits(planners[p].path()))
    r = _results(g)
    for p in range(P):
        n = int(r["off"][p + 1]) - int(r["off"][p])
        assert (n > 0) == (st[p] == capi.OK)
        if st[p] != capi.OK:
            assert r["raw"][p] == 0.0 and r["simp"][p] == 0.0 and r["checks"][p] == 0
    g.close()


# ------------------------------------------------------------------------------------------------ the pair matrix

@pytest.mark.parametrize("name", ["config1", "config2", "wall", "connect", "so3", "so3_bounded", "r6"])
def test_every_validity_bit_is_check_motions_verdict(name):
    g = batch(name)
    g.extract_paths()
    off, rows = g.paths()
    seen = set()
    problems = [p for p in range(g.n_problems) if off[p + 1] - off[p] >= 3][:8]
    assert len(problems) >= min(4, g.n_problems)
    for p in problems:
        path = rows[int(off[p]):int(off[p + 1])]
        L = len(path)
        for span in (0, 5):
            M = g.path_valid_matrix(p, span)
            S = sh.span_of(L, span)
            ii, jj = np.triu_indices(L, 2)
            keep = (jj - ii) <= S
            want = g.check_motion(path[ii[keep]], path[jj[keep]])
            assert np.array_equal(M[ii[keep], jj[keep]], want), (name, p, span)
            assert M[np.arange(L - 1), np.arange(1, L)].all()            # adjacent: true without a check
            assert not M[ii[~keep], jj[~keep]].any() and not np.tril(M).any()
            seen.update(want.tolist())
    assert seen == {True, False} or name == "so3"   # both verdicts occur (the fixture's one cone leaves every chord free)


# ------------------------------------------------------------------------------------------------ whole results

@pytest.fixture(scope="module")
def simplify_golden():
    with open(os.path.join(ROOT, "tests", "golden", "simplify_golden.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name, key", [("config1", "config1"), ("config2", "config2"), ("wall", "wall"), ("star", "config1_star"),
                                       ("so3", "so3_fixture")])
def test_golden_records_are_reproduced_bit_for_bit(simplify_golden, name, key):
    g = batch(name)
    g.extract_paths()
    raw_paths = _split(*g.paths())
    for span in (0, 3):
        r = _results(g, span)
        for rec in simplify_golden[key]:
            p, want = rec["pid"], rec["spans"][str(span)]
            assert len(raw_paths[p]) == rec["L"], (key, p)
            a, b = int(r["off"][p]), int(r["off"][p + 1])
            assert r["idx"][a:b].tolist() == want["idx"], (key, p, span)
            assert bits(r["raw"][p]) == bits(unhex(want["raw"])) and bits(r["simp"][p]) == bits(unhex(want["cost"])), (key, p, span)
            assert int(r["checks"][p]) == want["checks"]
            assert np.array_equal(bits(r["rows"][a:b]), bits(raw_paths[p][want["idx"]]))


@pytest.mark.parametrize("name, n", [("connect", 8), ("r6", 4), ("wall", 4)])
def test_python_dp_over_the_entry_points_verdicts_is_reproduced(name, n):
    g = batch(name)
    g.extract_paths()
    for span in (0, 2):
        _assert_equals_model(g, range(n), span)


def test_properties_on_every_solved_problem_of_256():
    g = _solved(scenarios.make_batch(scenarios.config2(), 256, 10000, True, SEED))
    g.extract_paths()
    raw_paths = _split(*g.paths())
    r = _results(g)
    fr, to = [], []
    shorter = 0
    for p in range(256):
        a, b = int(r["off"][p]), int(r["off"][p + 1])
        idx, rows, raw = r["idx"][a:b], r["rows"][a:b], raw_paths[p]
        assert len(raw) >= 2 and idx[0] == 0 and idx[-1] == len(raw) - 1          # the ends are kept
        assert (np.diff(idx.astype(np.int64)) > 0).all()
        assert np.array_equal(bits(rows), bits(raw[idx]))
        assert r["simp"][p] <= r["raw"][p]                                        # exactly: no tolerance
        shorter += r["simp"][p] < r["raw"][p]
        fr.append(rows[:-1])
        to.append(rows[1:])
    assert g.check_motion(np.concatenate(fr), np.concatenate(to)).all()          # every simplified edge passes
    assert shorter > 200
    g.close()


# ------------------------------------------------------------------------------------------------ shapes

def test_two_and_three_state_paths_built_with_set_tree():
    """goal_bias 1 and a max_distance that reaches the goal: one iteration appends the goal centre to the nearest node"""
    g = capi.RRTBatch(2, [(-10.0, 10.0)] * 2, 5.0, 1.0, 3, 100, 0.05, True, SEED)
    g.set_spheres([[0.0, 0.0]], [1.0])
    g.setup([[-4.0, 0.0], [-4.0, 5.0], [-4.0, -5.0]], [[4.0, 0.0], [4.0, 5.0], [0.0, -5.0]], 0.5)
    g.set_tree(0, [[-4.0, 0.0], [0.0, 3.0]], [-1, 0])     # (-4, 0) -> (4, 0) runs through the disc: the one pair is invalid
    g.set_tree(1, [[-4.0, 5.0], [0.0, 6.0]], [-1, 0])     # (-4, 5) -> (4, 5) is free: the one pair is valid
    with pytest.raises(capi.OxhipError):                  # set_tree dropped nothing that existed, and nothing exists yet
        g.paths()
    assert (g.solve(1) == capi.OK).all()
    r = _results(g)
    off, rows = g.paths()
    assert np.diff(off).tolist() == [3, 3, 2]
    assert [r["idx"][int(r["off"][p]):int(r["off"][p + 1])].tolist() for p in range(3)] == [[0, 1, 2], [0, 2], [0, 1]]
    assert r["checks"].tolist() == [1, 1, 0]
    assert bits(r["simp"][0]) == bits(r["raw"][0]) and r["simp"][1] < r["raw"][1] and bits(r["simp"][2]) == bits(r["raw"][2])
    assert bits(r["simp"][1]) == bits(capi.distance_batch([[-4.0, 5.0]], [[4.0, 5.0]])[0])
    assert g.path_valid_matrix(0)[0, 2] == False and g.path_valid_matrix(1)[0, 2] == True  # noqa: E712
    for span in (1, 2):
        r2 = _results(g, span)
        assert r2["idx"].tolist() == ([0, 1, 2, 0, 1, 2, 0, 1] if span == 1 else r["idx"].tolist())
    g.close()


def test_a_path_of_hundreds_of_states_and_every_span():
    """max_distance 0.05 on config 1: longer than 64 states and than a workgroup's 256 pair slots"""
    sc = dict(scenarios.config1(), max_distance=0.05)
    g = _solved(scenarios.make_batch(sc, 2, 60000, True, SEED), 10 ** 7)
    g.extract_paths()
    off, rows = g.paths()
    assert (np.diff(off) > 256).all()
    for p in range(2):
        assert np.array_equal(bits(rows[int(off[p]):int(off[p + 1])]), bits(g.path(p)))
    _assert_equals_model(g, range(2), 16)
    for span in (1, 2):
        _assert_equals_model(g, [0], span)
    r = _results(g, 1)
    assert r["idx"].tolist() == list(range(int(off[1]))) + list(range(int(off[2] - off[1])))
    assert np.array_equal(bits(r["simp"]), bits(r["raw"])) and (r["checks"] == 0).all()
    g.close()


def test_full_span_on_the_long_batches_scene_sizes():
    """span 0 on ordinary paths, and the batch-wide figures: costs drop, and the checks are the pair count"""
    g = batch("config1")
    g.extract_paths()
    L = np.diff(g.paths()[0]).astype(np.int64)
    r = _results(g)
    assert r["checks"].tolist() == [(l - 1) * (l - 2) // 2 for l in L]
    assert (r["simp"] < r["raw"]).all()


@pytest.mark.parametrize("name", ["config2", "so3"])
def test_the_round_size_never_changes_the_output(name):
    g = batch(name)
    ref = _results(g, 0, 0)
    assert g.paths_last_timing()["rounds"] == 1
    for chunk in (1, 7):
        got = _results(g, 0, chunk)
        assert g.paths_last_timing()["rounds"] == -(-g.n_problems // chunk)
        for k in ref:
            assert np.array_equal(ref[k].view(np.uint64) if ref[k].dtype == np.float64 else ref[k],
                                  got[k].view(np.uint64) if got[k].dtype == np.float64 else got[k]), (chunk, k)


def test_without_obstacles_every_pair_is_valid():
    g = batch("free")
    r = _results(g)
    off, rows = g.paths()
    for p in range(g.n_problems):
        L = int(off[p + 1] - off[p])
        assert r["idx"][int(r["off"][p]):int(r["off"][p + 1])].tolist() == [0, L - 1]
        assert bits(r["simp"][p]) == bits(capi.distance_batch(rows[int(off[p])][None], rows[int(off[p + 1]) - 1][None])[0])
        assert g.path_valid_matrix(p)[np.triu_indices(L, 1)].all()


# ------------------------------------------------------------------------------------------------ life cycle

def _raises(status, fn, *args):
    with pytest.raises(capi.OxhipError) as ei:
        fn(*args)
    assert ei.value.status == status, ei.value
    return str(ei.value)


def test_results_live_until_the_trees_change():
    sc = scenarios.config1()
    g = scenarios.make_batch(sc, 4, 10000, True, SEED)
    assert "no extracted" in _raises(capi.ERR_BAD_ARG, g.paths)
    assert "no simplified" in _raises(capi.ERR_BAD_ARG, g.simplified_paths)
    g.solve(sh.BUDGET)
    _raises(capi.ERR_BAD_ARG, g.paths)
    before = (g.counts(), [g.tree(p) for p in range(4)])
    g.extract_paths()
    total = len(g.paths()[1])
    _raises(capi.ERR_BAD_ARG, g.simplified_paths)          # extracted, not simplified
    g.simplify_paths()
    g.simplified_paths()
    # both calls leave trees, counts and checksums as they were
    after = (g.counts(), [g.tree(p) for p in range(4)])
    for k in before[0]:
        assert np.array_equal(before[0][k], after[0][k]), k
    for (s0, p0), (s1, p1) in zip(before[1], after[1]):
        assert np.array_equal(bits(s0), bits(s1)) and np.array_equal(p0, p1)
    # a buffer too small: ERR_CAPACITY with the total set
    L = capi.lib()
    import ctypes as C
    tot = C.c_uint64()
    small = np.zeros((total - 1, 2))
    assert L.oxhip_rrt_batch_get_paths(g._h, None, small.ctypes.data_as(C.POINTER(C.c_double)), total - 1, C.byref(tot)) == capi.ERR_CAPACITY
    assert tot.value == total
    tot = C.c_uint64()
    assert L.oxhip_rrt_batch_get_simplified_paths(g._h, None, small.ctypes.data_as(C.POINTER(C.c_double)), None, 1, C.byref(tot)) == capi.ERR_CAPACITY
    assert tot.value == int(g.simplified_paths()[0][-1]) > 1
    # a later solve / set_tree / setup discards the results: never a stale row
    g.solve(1)
    _raises(capi.ERR_BAD_ARG, g.paths)
    _raises(capi.ERR_BAD_ARG, g.simplified_paths)
    g.simplify_paths()                                     # extracts by itself
    assert len(g.paths()[1]) == total and len(g.simplified_paths()[1]) > 0
    states, parents = g.tree(0)
    g.set_tree(0, states, parents)
    _raises(capi.ERR_BAD_ARG, g.paths)
    _raises(capi.ERR_BAD_ARG, g.simplified_paths)
    g.simplify_paths()
    g.setup(sc["start"], sc["goal_centre"], sc["goal_radius"])
    _raises(capi.ERR_BAD_ARG, g.paths)
    _raises(capi.ERR_BAD_ARG, g.simplified_paths)
    g.extract_paths()
    assert len(g.paths()[1]) == 0 and g.paths()[0].tolist() == [0] * 5     # set up, nothing solved: every length 0
    g.close()


@pytest.mark.parametrize("name", ["se2", "se3"])
def test_se2_and_se3_are_not_built(name):
    g = batch(name)
    assert "not built" in _raises(capi.ERR_BAD_ARG, g.simplify_paths)
    assert "not built" in _raises(capi.ERR_BAD_ARG, g.path_valid_matrix, 0)
    g.extract_paths()                                      # extraction is
    assert len(g.paths()[1]) > 0


# ------------------------------------------------------------------------------------------------ the Python surface

def test_simplify_solution_on_the_readme_scene_and_the_so3_fixture():
    from oxmpl_amd.base import (Path, ProblemDefinition, RealVectorState, RealVectorStateSpace, SO3ConeValidityChecker, SO3State,
                                SO3StateSpace, SphereBoxValidityChecker)
    from oxmpl_amd.geometric import RRT, RRTConnect, RRTStar

    class Goal:
        def __init__(self, target, radius):
            self.target, self.radius = target, radius

    sc = scenarios.config1()
    space = RealVectorStateSpace(dimension=2, bounds=sc["bounds"])
    pd = ProblemDefinition.from_real_vector(space, RealVectorState(sc["start"]), Goal(RealVectorState(sc["goal_centre"]), 0.5))
    checker = SphereBoxValidityChecker(spheres=[([0.0, 0.0], 2.0)], boxes=[])
    for make in (lambda: RRT(0.5, 0.05, pd), lambda: RRTConnect(0.5, 0.05, pd), lambda: RRTStar(0.5, 0.05, 1.0, pd)):
        planner = make()
        with pytest.raises(Exception, match="setup"):
            planner.simplify_solution()
        planner.setup(checker)
        with pytest.raises(Exception, match="No solution found"):
            planner.simplify_solution()
        raw = planner.solve(5.0)
        short = planner.simplify_solution()
        assert isinstance(short, Path) and all(isinstance(s, RealVectorState) for s in short.states)
        rv, sv = np.array([s.values for s in raw.states]), np.array([s.values for s in short.states])
        assert 2 <= len(sv) < len(rv)
        assert np.array_equal(bits(sv[0]), bits(rv[0])) and np.array_equal(bits(sv[-1]), bits(rv[-1]))
        pos = [int(np.flatnonzero((bits(rv) == bits(s)).all(axis=1))[0]) for s in sv]     # waypoints of the raw path, in order
        assert pos == sorted(set(pos))
        length = lambda v: float(np.sum(np.sqrt(np.sum(np.diff(v, axis=0) ** 2, axis=1))))  # noqa: E731
        assert length(sv) <= length(rv) * (1.0 + 1e-12)
        assert planner._batch.check_motion(sv[:-1], sv[1:]).all()
        assert len(planner.simplify_solution(max_span=1).states) == len(rv)

    fx = so3.fixture_scene()
    sspace = SO3StateSpace()
    spd = ProblemDefinition.from_so3(sspace, SO3State(*fx["start"]), Goal(SO3State(*fx["target"]), math.radians(10.0)))
    planner = RRT(0.5, 0.0, spd)
    planner.setup(SO3ConeValidityChecker([(SO3State.identity(), math.radians(44.9))]))
    raw = planner.solve(5.0)
    short = planner.simplify_solution()
    assert isinstance(short, Path) and all(isinstance(s, SO3State) for s in short.states)
    assert 2 <= len(short.states) <= len(raw.states)
    assert short.states[0].values == raw.states[0].values and short.states[-1].values == raw.states[-1].values
    assert so3.is_so3_path_valid([s.values for s in short.states], so3.Cones(fx["cones"]), fx["fraction"])


def test_simplify_solution_is_a_type_error_on_se3():
    from oxmpl_amd.base import ProblemDefinition, SE3RigidBodyValidityChecker, SE3State, SE3StateSpace
    from oxmpl_amd.geometric import RRTConnect

    class Goal:
        def __init__(self, target, radius):
            self.target, self.radius = target, radius

    sc = scenarios.se3_field()
    space = SE3StateSpace(sc["bounds"])
    pd = ProblemDefinition.from_se3(space, SE3State.from_values(sc["start"]), Goal(SE3State.from_values(sc["goal_centre"]), sc["goal_radius"]))
    planner = RRTConnect(sc["max_distance"], sc["goal_bias"], pd)
    planner.setup(SE3RigidBodyValidityChecker(list(zip(sc["body"][0].tolist(), sc["body"][1].tolist())),
                                              list(zip(sc["spheres"][0].tolist(), sc["spheres"][1].tolist()))))
    planner.solve(10.0)
    with pytest.raises(TypeError):
        planner.simplify_solution()
