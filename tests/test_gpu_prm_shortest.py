"""GPU: a batch of PRM queries answered with shortest paths (oxhip_prm_solve_batch_shortest, prm_shortest.hip, DESIGN.md section
19) against the pure-Python checker (tests/golden/make_golden_prm_shortest.py: Dijkstra, then breadth-first levels over the tight
edges), the golden file it wrote, and the breadth-first batch on the same handle.  Every comparison is bit for bit: statuses,
costs, node lists, rows, and for some queries every milestone's label, hops and parent."""
import json
import math
import os
import sys

import numpy as np
import pytest

from helpers import unhex, hexf, bits
from prm_helpers import STATUS_NAME

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden as mg  # noqa: E402
import make_golden_prm_shortest as gsp  # noqa: E402
import make_golden_prm_so3 as gp3  # noqa: E402
import make_golden_so3 as g3  # noqa: E402

pytestmark = pytest.mark.gpu

from oxmpl_amd import capi  # noqa: E402
from prm_shortest_helpers import Batch, RoadmapChecker, make_gpu_prm, DISTANCE, UNIT, ZERO  # noqa: E402

SEED = 20261019
FIXTURE = [0.0, 0.0, 0.0, 1.0, math.pi]
SCENES = ("wall", "r6", "fixture")


def _golden(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return json.load(f)


def make_so3_prm(sc, **kw):
    bounds = FIXTURE if sc["bounds"] is None else list(sc["bounds"][0]) + [sc["bounds"][1]]
    args = dict(lvs_fraction=sc["fraction"], max_samples=sc["max_samples"], seed=sc["seed"], stream=sc["stream"], space=capi.SPACE_SO3)
    args.update(kw)
    g = capi.PRMRoadmap(4, bounds, sc["radius"], sc["max_milestones"], **args)
    if sc["cones"]:
        g.set_spheres([c for c, _ in sc["cones"]], [r for _, r in sc["cones"]])
    return g


class Scene(RoadmapChecker):
    """a golden scene's roadmap on the device, its copy for the checker, and the scene's 32 recorded queries"""

    def __init__(self, name):
        self.name = name
        qs = _golden("prm_batch_golden.json")[name]["queries"]
        self.bfs_golden = qs
        self.starts = [[unhex(v) for v in q["start"]] for q in qs]
        self.goals = [[unhex(v) for v in q["goal_c"]] for q in qs]
        self.radii = [unhex(q["goal_r"]) for q in qs]
        self.so3 = name == "fixture"
        self.dist = g3.distance if self.so3 else mg.distance
        self.g = make_so3_prm(gp3.scenes()["fixture"]) if self.so3 else make_gpu_prm(_golden("prm_golden.json")[name]["params"])
        self.g.setup(self.starts[0], self.goals[0], self.radii[0])
        self.g.construct_roadmap()
        self.load_roadmap()

    def random_queries(self, n, seed):
        rng = np.random.default_rng([SEED, seed])
        if self.so3:
            starts = [g3.normalise([float(v) for v in row]) for row in rng.standard_normal(size=(n, 4))]
            goals = [g3.normalise([float(v) for v in row]) for row in rng.standard_normal(size=(n, 4))]
            return starts, goals, [float(v) for v in rng.uniform(0.2, 0.6, size=n)]
        dim = self.g.dim
        r_lo, r_hi = (0.3, 0.8) if dim == 2 else (2.0, 3.5)
        return (rng.uniform(0.0, 10.0, size=(n, dim)).tolist(), rng.uniform(0.0, 10.0, size=(n, dim)).tolist(),
                [float(v) for v in rng.uniform(r_lo, r_hi, size=n)])


_scenes = {}


@pytest.fixture(scope="module", params=SCENES)
def scene(request):
    if request.param not in _scenes:
        _scenes[request.param] = Scene(request.param)
    return _scenes[request.param]


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for s in _scenes.values():
        s.g.close()
    _scenes.clear()


@pytest.fixture(scope="module")
def golden_batches(scene):
    """the scene's 32 recorded queries: the breadth-first batch, then the three shortest-path batches"""
    s = scene
    bfs = Batch(s.g, s.starts, s.goals, s.radii, weights=None)
    return bfs, {mode: Batch(s.g, s.starts, s.goals, s.radii, weights=mode) for mode in (UNIT, ZERO, DISTANCE)}


# ------------------------------------------------------------------------------------------------ 1. the golden file
def test_golden_scene_in_one_batch(scene, golden_batches):
    s = scene
    rec = _golden("prm_shortest_golden.json")[s.name]
    assert s.n == rec["n"] and len(rec["queries"]) == 32
    _, B = golden_batches
    for mode, key in ((DISTANCE, "nodes"), (UNIT, "nodes_unit")):
        B[mode].check_rows_are_milestones(s.states)
        for k, r in enumerate(rec["queries"]):
            assert STATUS_NAME[int(B[mode].status[k])] == r["status"], k
            assert B[mode].path_nodes(k)[1:] == r["nodes" if mode == DISTANCE else "nodes_unit"], (k, key)
            if mode == DISTANCE:
                assert hexf(B[mode].cost[k]) == r["cost"], k
            elif r["status"] == "solved":
                assert B[mode].cost[k] == float(len(r["nodes_unit"]))      # every weight and every init is 1.0
    assert sum(r["status"] == "solved" for r in rec["queries"]) == gsp.SOLVED_COUNTS[s.name]


def test_statuses_and_query_sets_are_the_bfs_batch_s(scene, golden_batches):
    bfs, B = golden_batches
    for mode in (DISTANCE, UNIT, ZERO):
        for a, b in ((B[mode].status, bfs.status), (B[mode].ns, bfs.ns), (B[mode].ng, bfs.ng)):
            assert np.array_equal(a, b)
    for k, q in enumerate(scene.bfs_golden):
        assert STATUS_NAME[int(bfs.status[k])] == q["status"]
        want_sets = (0, 0) if q["status"] == "invalid_start" else (q["n_start"], q["n_goal"])
        assert (int(B[DISTANCE].ns[k]), int(B[DISTANCE].ng[k])) == want_sets, k


def test_unit_and_zero_weights_agree_and_have_the_bfs_length(scene, golden_batches):
    bfs, B = golden_batches
    assert np.array_equal(B[UNIT].nodes, B[ZERO].nodes) and np.array_equal(B[UNIT].off, B[ZERO].off)
    assert np.array_equal(bits(B[UNIT].rows), bits(B[ZERO].rows)) and np.array_equal(B[UNIT].goal, B[ZERO].goal)
    assert np.array_equal(B[UNIT].len, bfs.len) and np.array_equal(B[ZERO].len, bfs.len)
    ok = bfs.status == capi.OK
    assert np.all(B[ZERO].cost[ok] == 0.0) and np.array_equal(B[UNIT].cost[ok], bfs.len[ok].astype(np.float64) - 1.0)
    assert np.all(B[DISTANCE].len >= bfs.len)


# ------------------------------------------------------------------------------------------------ 2. every label
def test_all_labels_of_four_queries(scene):
    s = scene
    for mode in (DISTANCE, UNIT, ZERO):
        B = Batch(s.g, s.starts, s.goals, s.radii, weights=mode)
        solved = [int(q) for q in np.nonzero(B.status == capi.OK)[0]]
        dry = [int(q) for q in np.nonzero(B.status == capi.ERR_NO_SOLUTION_FOUND)[0]]
        for q in solved[:2] + solved[-1:] + dry[:1]:
            res = s.checker(B, q, mode)
            cost, hops, parent = s.g.batch_labels(q)
            assert np.array_equal(bits(cost), bits(np.array(res["c"], dtype=np.float64))), (mode, q)
            assert [int(v) for v in hops] == res["hops"] and [int(v) for v in parent] == res["parent"], (mode, q)
            assert np.array_equal(np.isinf(cost), hops == gsp.UNSET)
        invalid = np.nonzero(B.status == capi.ERR_INVALID_START_STATE)[0]
        if len(invalid):
            cost, hops, parent = s.g.batch_labels(int(invalid[0]))
            assert np.all(np.isinf(cost)) and np.all(hops == gsp.UNSET) and np.all(parent == gsp.UNSET)
    with pytest.raises(capi.OxhipError) as ei:                 # cap < n
        h = np.zeros(s.n, dtype=np.uint32)
        capi._check(capi.lib().oxhip_prm_batch_get_labels(s.g._h, 0, None, capi._p(h, capi._u32p), None, s.n - 1))
    assert ei.value.status == capi.ERR_CAPACITY
    capi._check(capi.lib().oxhip_prm_batch_get_labels(s.g._h, 0, None, None, None, 0))     # nothing asked for


# ------------------------------------------------------------------------------------------------ 3. random queries
def test_64_random_queries_against_the_checker(scene):
    s = scene
    starts, goals, radii = s.random_queries(64, 1)
    bfs = Batch(s.g, starts, goals, radii, weights=None)
    for mode in (DISTANCE, UNIT):
        B = Batch(s.g, starts, goals, radii, weights=mode)
        B.check_rows_are_milestones(s.states)
        for a, b in ((B.status, bfs.status), (B.ns, bfs.ns), (B.ng, bfs.ng)):
            assert np.array_equal(a, b)
        solved = s.check_against_checker(B, mode)
        assert solved == int(np.sum(bfs.status == capi.OK)) and 8 <= solved
        if mode == DISTANCE:                                   # the path's left-to-right cost is its label, and no more than BFS's
            for q in np.nonzero(B.status == capi.OK)[0]:
                assert gsp.path_cost(B.starts[q], B.path_nodes(q)[1:], s.states, s.dist) == B.cost[q]
                assert B.cost[q] <= gsp.path_cost(B.starts[q], bfs.path_nodes(q)[1:], s.states, s.dist)
        else:
            assert np.array_equal(B.len, bfs.len)
    stats = s.g.batch_search_stats()
    assert len(stats["label_rounds"]) == 64 and np.all(stats["label_rounds"][bfs.status == capi.OK] >= 1)
    assert np.all(stats["label_rounds"] <= s.n)


# ------------------------------------------------------------------------------------------------ 4. chunking, order, company
def test_results_do_not_depend_on_chunking_order_or_company(scene, golden_batches):
    s = scene
    ref = golden_batches[1][DISTANCE]
    assert ref.timing["rounds"] == 1
    for chunk, rounds in ((1, 32), (7, 5), (0, 1)):
        B = Batch(s.g, s.starts, s.goals, s.radii, chunk_queries=chunk)
        assert B.timing["rounds"] == rounds
        B.same_as(ref)
    for q in range(32):                                        # each query as a batch of one
        one = Batch(s.g, s.starts[q:q + 1], s.goals[q:q + 1], s.radii[q:q + 1])
        assert one.status[0] == ref.status[q] and one.goal[0] == ref.goal[q] and (one.ns[0], one.ng[0]) == (ref.ns[q], ref.ng[q])
        assert bits(one.cost[0]) == bits(ref.cost[q])
        assert one.path_nodes(0) == ref.path_nodes(q) and np.array_equal(bits(one.rows), bits(ref.path(q)))
    rev = Batch(s.g, s.starts[::-1], s.goals[::-1], s.radii[::-1])
    for a, b in ((rev.status, ref.status), (rev.len, ref.len), (rev.goal, ref.goal), (rev.ns, ref.ns), (rev.ng, ref.ng), (bits(rev.cost), bits(ref.cost))):
        assert np.array_equal(a[::-1], b)
    for q in range(32):
        assert rev.path_nodes(31 - q) == ref.path_nodes(q) and np.array_equal(bits(rev.path(31 - q)), bits(ref.path(q)))


def test_timeout_leaves_a_suffix_unanswered(scene, golden_batches):
    s = scene
    ref = golden_batches[1][DISTANCE]
    for timeout in (2e-6, 3600.0):
        B = Batch(s.g, s.starts, s.goals, s.radii, timeout_s=timeout, chunk_queries=1)
        timed_out = B.status == capi.ERR_TIMEOUT
        first = int(np.argmax(timed_out)) if timed_out.any() else 32
        assert first >= 1 and np.all(timed_out[first:]) and not timed_out[:first].any()      # a suffix; the first round always runs
        assert B.timing["rounds"] == first and np.all(B.len[first:] == 0) and np.all(np.isinf(B.cost[first:]))
        B.same_as(ref, upto=first)
        assert len(B.nodes) == int(ref.off[first])
    assert first == 32                                         # an hour is enough


# ------------------------------------------------------------------------------------------------ 5. statuses of the getters
def test_getters_refuse_what_they_should(scene):
    s = scene
    with pytest.raises(capi.OxhipError) as ei:
        s.g.solve_batch_shortest(s.starts, s.goals, s.radii, weights=3)
    assert ei.value.status == capi.ERR_BAD_ARG
    with pytest.raises(capi.OxhipError) as ei:
        s.g.solve_batch_shortest([[float("nan")] * s.g.dim], s.goals[:1], s.radii[:1])
    assert ei.value.status == capi.ERR_BAD_ARG
    Batch(s.g, s.starts, s.goals, s.radii, weights=None)
    for call in (s.g.batch_costs, lambda: s.g.batch_labels(0), s.g.batch_search_stats):      # the last batch was breadth-first
        with pytest.raises(capi.OxhipError) as ei:
            call()
        assert ei.value.status == capi.ERR_BAD_ARG
    empty = Batch(s.g, np.zeros((0, s.g.dim)), np.zeros((0, s.g.dim)), np.zeros(0))
    assert len(empty.status) == 0 and len(empty.cost) == 0 and empty.timing["rounds"] == 0


# ------------------------------------------------------------------------------------------------ 6. non-interference
def test_a_shortest_batch_leaves_the_handle_and_the_bfs_batch_as_they_were(scene, golden_batches):
    s = scene
    k = int(np.nonzero(golden_batches[0].status == capi.OK)[0][0])
    s.g.set_problem(s.starts[k], s.goals[k], s.radii[k])
    st0, path0 = s.g.solve()
    sc0, gi0 = (a.copy() for a in s.g.query_sets())
    bfs0 = Batch(s.g, s.starts, s.goals, s.radii, weights=None)
    for mode in (DISTANCE, UNIT, ZERO):
        Batch(s.g, s.starts, s.goals, s.radii, weights=mode)
    sc1, gi1 = s.g.query_sets()                                # the last single solve's sets, not a batch's
    assert np.array_equal(sc0, sc1) and np.array_equal(gi0, gi1)
    st1, path1 = s.g.solve()                                   # the handle's own problem definition
    assert st1 == st0 == capi.OK and np.array_equal(bits(path0), bits(path1))
    Batch(s.g, s.starts, s.goals, s.radii, weights=None).same_as(bfs0)
    bfs0.same_as(golden_batches[0])


# ------------------------------------------------------------------------------------------------ 7. the weights cache
def test_setup_drops_the_batch_and_the_edge_weights():
    """The seed belongs to the handle's configuration, so the second roadmap on the same handle gets other obstacles instead:
    other milestones, other edges, other weights."""
    s = Scene("r6")
    try:
        starts, goals, radii = s.random_queries(32, 2)
        before = Batch(s.g, starts, goals, radii)
        assert s.check_against_checker(before, DISTANCE) >= 4
        old_states, old_entries = s.states.copy(), s.g.sizes()[1]
        s.g.setup(starts[0], goals[0], radii[0])
        for call in (s.g.batch_costs, lambda: s.g.batch_labels(0), s.g.batch_results, s.g.batch_search_stats):
            with pytest.raises(capi.OxhipError) as ei:
                call()
            assert ei.value.status == capi.ERR_UNSAMPLED_STATE_SPACE
        rng = np.random.default_rng(77)
        s.g.set_spheres(rng.uniform(1.0, 9.0, size=(10, 6)), rng.uniform(2.0, 3.0, size=10))
        s.g.construct_roadmap()
        s.load_roadmap()
        assert s.g.sizes()[1] != old_entries and not np.array_equal(bits(s.states), bits(old_states))
        after = Batch(s.g, starts, goals, radii)
        after.check_rows_are_milestones(s.states)
        assert s.check_against_checker(after, DISTANCE) >= 4   # the new roadmap's answers, from the new roadmap's weights
        assert not np.array_equal(bits(after.cost), bits(before.cost))
    finally:
        s.g.close()


# ------------------------------------------------------------------------------------------------ 8. the Python class surface
def test_python_surface_solve_batch_shortest_on_the_wall_scene():
    from oxmpl_amd.base import ProblemDefinition, RealVectorState, RealVectorStateSpace, SphereBoxValidityChecker
    from oxmpl_amd.geometric import PRM, _MESSAGES

    class Goal:
        def __init__(self, target, radius):
            self.target, self.radius = target, radius

    P = _golden("prm_golden.json")["wall"]["params"]
    space = RealVectorStateSpace(2, [tuple(b) for b in P["bounds"]])

    def problem(start, goal, r):
        return ProblemDefinition(space, RealVectorState(start), Goal(RealVectorState(goal), r))

    planner = PRM(5.0, 0.5, problem([1.0, 5.0], [9.0, 5.0], 0.5), max_milestones=1500, seed=3)
    planner.setup(SphereBoxValidityChecker(boxes=[(lo, hi) for lo, hi in P["boxes"]]))
    planner.construct_roadmap()
    pds = [problem([1.0, 5.0], [9.0, 5.0], 0.5), problem([5.0, 5.0], [9.0, 5.0], 0.5), problem([1.0, 5.0], [20.0, 20.0], 0.5),
           problem([9.0, 9.0], [1.0, 1.0], 0.4)]
    bfs = planner.solve_batch(pds, 5.0)
    out = planner.solve_batch(pds, 5.0, shortest=True)
    assert len(out) == 4
    costs = planner._prm.batch_costs()

    def length(path):
        rows = [st.values for st in path.states]
        c = mg.distance(rows[0], rows[1])
        for a, b in zip(rows[1:], rows[2:]):
            c = c + mg.distance(a, b)
        return c

    for k in (0, 3):
        rows = [st.values for st in out[k].states]
        assert isinstance(out[k].states[0], RealVectorState) and len(rows) >= len(bfs[k].states) >= 2
        assert list(rows[0]) == list(pds[k].start_state.values)
        assert mg.distance(rows[-1], pds[k].goal.target.values) <= pds[k].goal.radius
        assert length(out[k]) == costs[k] <= length(bfs[k])
    assert length(out[0]) < length(bfs[0]) or length(out[3]) < length(bfs[3])
    assert isinstance(out[1], Exception) and str(out[1]) == _MESSAGES[capi.ERR_INVALID_START_STATE]
    assert isinstance(out[2], Exception) and str(out[2]) == _MESSAGES[capi.ERR_NO_SOLUTION_FOUND]
    again = planner.solve_batch(pds, 5.0)                      # the default is still the breadth-first batch
    for k in (0, 3):
        assert np.array_equal(bits([st.values for st in again[k].states]), bits([st.values for st in bfs[k].states]))
