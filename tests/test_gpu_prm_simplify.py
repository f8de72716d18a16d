"""GPU: the PRM handle's own checker (oxhip_prm_is_valid / _check_motion) and the dense shortcut of a batch's answered paths
(oxhip_prm_batch_simplify_paths, prm_path_simplify.hip), bit for bit against the model of
tests/prm_simplify_helpers.py over the CPU side's check_motion, distance and interpolate: the oracle for R^n, the checker of
tests/golden/make_golden_prm_so3.py for SO(3).  Small roadmaps (at most 2,000 milestones) or planted chains, at most 64 queries."""
import math
import os
import sys

import numpy as np
import pytest

from oxmpl_amd import capi, scenarios
from oracle import oracle_py as orc
from helpers import bits
import prm_simplify_helpers as ph

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_prm_so3 as gp  # noqa: E402
import make_golden_so3 as g3  # noqa: E402

pytestmark = pytest.mark.gpu
SO3_BOUNDS = [0.0, 0.0, 0.0, 1.0, math.pi]


def _expect(status, call):
    with pytest.raises(capi.OxhipError) as ei:
        call()
    assert ei.value.status == status, ei.value
    return str(ei.value)


class Side:
    """the CPU side of one scene: valid(a, b), dist, interp, is_valid over rows"""

    def __init__(self, valid, dist, interp, is_valid):
        self.valid, self.dist, self.interp, self.is_valid = valid, dist, interp, is_valid


def rn_side(dim, bounds, fraction, spheres=None, boxes=None):
    o = orc.OracleRRT(dim, bounds, 0.5, 0.0, fraction, 16, True, 1, 0)
    if spheres is not None and len(spheres[1]):
        o.set_spheres(np.asarray(spheres[0], dtype=np.float64).reshape(-1, dim), np.asarray(spheres[1], dtype=np.float64))
    if boxes is not None:
        o.set_boxes(np.asarray(boxes[0], dtype=np.float64), np.asarray(boxes[1], dtype=np.float64))
    o.setup([0.5 * (lo + hi) for lo, hi in bounds], [lo for lo, _ in bounds], 0.1)
    side = Side(lambda a, b: bool(o.check_motion(a, b)), orc.distance, orc.interpolate, lambda p: bool(o.is_valid(p)))
    side.keep = o
    return side


def so3_side(cones, fraction):
    c = g3.Cones(cones)
    return Side(lambda a, b: bool(g3.check_motion(c, fraction, list(a), list(b))), lambda a, b: g3.distance(list(a), list(b)),
                lambda a, b, t: g3.interpolate(list(a), list(b), t), lambda p: bool(c.is_valid(list(p))))


def batch_of(g, starts, goals, radii, weights=None, **kw):
    if weights is None:
        status = g.solve_batch(starts, goals, radii, **kw).copy()
    else:
        status = g.solve_batch_shortest(starts, goals, radii, weights=weights, **kw).copy()
    off, nodes, rows = g.batch_paths()
    return status, off, rows


def raw_path(off, rows, q):
    return rows[int(off[q]):int(off[q + 1])]


def simplified(g, m, span, chunk=0):
    g.simplify_batch_paths(m, span, chunk)
    off, states, idx = g.simplified_batch_paths()
    res = g.simplify_results()
    return off, states, idx, res


def check_against_model(g, side, status, off, rows, m, span, queries=None, chunk=0):
    """dense indices, states, both costs and checks of every query against the model; -> the number of answered queries compared"""
    soff, states, idx, res = simplified(g, m, span, chunk)
    assert len(soff) == len(status) + 1 and int(soff[0]) == 0 and len(idx) == int(soff[-1]) == len(states)
    compared = 0
    for q in range(len(status)):
        a, b = int(soff[q]), int(soff[q + 1])
        if status[q] != capi.OK:
            assert a == b and res["raw_cost"][q] == 0.0 and res["simplified_cost"][q] == 0.0 and res["checks"][q] == 0, q
            continue
        path = raw_path(off, rows, q)
        assert int(res["checks"][q]) == ph.expected_checks(len(path), m, span), q
        assert int(idx[a]) == 0 and int(idx[b - 1]) == (len(path) - 1) * m and res["simplified_cost"][q] <= res["raw_cost"][q]
        assert np.array_equal(bits(states[a]), bits(path[0])) and np.array_equal(bits(states[b - 1]), bits(path[-1]))
        if queries is not None and q not in queries:
            continue
        model = ph.dense_shortcut(path, m, span, side.valid, side.dist, side.interp)
        assert [int(v) for v in idx[a:b]] == model["idx"], (q, m, span)
        assert np.array_equal(bits(states[a:b]), bits(np.array([model["dense"][u] for u in model["idx"]]))), (q, m, span)
        assert bits(np.float64(res["raw_cost"][q])) == bits(np.float64(model["raw"])), (q, m, span)
        assert bits(np.float64(res["simplified_cost"][q])) == bits(np.float64(model["simp"])), (q, m, span)
        assert int(res["checks"][q]) == model["checks"]
        compared += 1
    return compared


def check_matrix(g, side, path, q, m, span):
    """the hook's matrix against the CPU verdict of every checked pair, 1 on same-edge pairs, 0 outside the window"""
    got = g.batch_path_valid_matrix(q, m, span)
    dense = ph.dense_points(path, m, side.interp)
    M, W = len(dense), ph.span_of(len(path), span) * m
    assert got.shape == (M, M)
    want = np.zeros((M, M), dtype=bool)
    for u in range(M):
        for v in range(u + 1, min(M, u + W + 1)):
            want[u, v] = True if ph.same_edge(u, v, m) else side.valid(dense[u], dense[v])
    assert np.array_equal(got, want), (q, m, span)
    return want


# ------------------------------------------------------------------------------------------------ scenes

R2 = dict(dim=2, bounds=[(0.0, 10.0), (0.0, 10.0)], radius=1.2, fraction=0.05, n=400, seed=9, stream=2,
          spheres=(np.array([[3.0, 3.0], [6.5, 6.0], [3.0, 7.5], [7.0, 2.5], [5.0, 4.5]]), np.array([1.2, 1.4, 1.0, 1.1, 0.6])))


def r2_queries():
    starts = [[0.5, 0.5], [9.5, 9.5], [3.0, 3.0], [0.5, 9.5], [9.5, 0.5], [5.0, 9.5], [1.0, 5.0], [5.0, 0.6], [8.9, 5.1], [2.0, 9.0]]
    goals = [[9.5, 9.5], [0.5, 0.5], [9.0, 9.0], [9.5, 0.5], [0.5, 9.5], [5.0, 0.5], [30.0, 30.0], [5.0, 9.4], [1.0, 5.0], [8.0, 1.0]]
    return np.array(starts), np.array(goals), np.array([0.6] * 6 + [1e-3] + [0.6] * 3)   # query 2: invalid start; 6: no goal


@pytest.fixture(scope="module")
def r2():
    g = capi.PRMRoadmap(2, R2["bounds"], R2["radius"], R2["n"], lvs_fraction=R2["fraction"], seed=R2["seed"], stream=R2["stream"])
    g.set_spheres(*R2["spheres"])
    g.setup([0.5, 0.5], [9.5, 9.5], 0.6)
    g.construct_roadmap()
    o = orc.OraclePRM(2, R2["bounds"], R2["radius"], lvs_fraction=R2["fraction"], seed=R2["seed"], stream=R2["stream"])
    o.set_spheres(*R2["spheres"])
    o.setup([0.5, 0.5], [9.5, 9.5], 0.6)
    o.construct_roadmap(R2["n"])
    yield g, o, rn_side(2, R2["bounds"], R2["fraction"], R2["spheres"])
    g.close()


@pytest.fixture(scope="module")
def r6():
    sc = scenarios.config5()
    g = scenarios.make_prm(sc, 2000, connection_radius=4.0)     # (at config 5's own radius 2,000 milestones answer nothing)
    g.construct_roadmap()
    rng = np.random.default_rng(5)
    starts = np.vstack([sc["start"], np.array(sc["start"]) + rng.uniform(-0.3, 0.3, (3, 6)), np.array(sc["goal_centre"]) + rng.uniform(-0.3, 0.3, (4, 6))])
    goals = np.vstack([[sc["goal_centre"]] * 4, [sc["start"]] * 4])
    yield g, starts, goals, np.full(8, 1.5), rn_side(6, sc["bounds"], sc["lvs_fraction"], sc["spheres"])
    g.close()


SO3 = gp.scenes()["bounded"]


@pytest.fixture(scope="module")
def so3():
    sc = SO3
    g = capi.PRMRoadmap(4, list(sc["bounds"][0]) + [sc["bounds"][1]], sc["radius"], 300, lvs_fraction=sc["fraction"], seed=sc["seed"],
                        stream=sc["stream"], space=capi.SPACE_SO3)
    g.set_spheres([c for c, _ in sc["cones"]], [r for _, r in sc["cones"]])
    s, t, gr = sc["queries"][0]
    g.setup(s, t, gr)
    g.construct_roadmap()
    inside = sc["cones"][0][0]                                   # a start inside a cone: not answered
    starts = np.array([s, t, inside, g3.normalise([0.2, 0.1, -0.2, 0.9])])
    goals = np.array([t, s, t, s])
    yield g, starts, goals, np.full(4, gr), so3_side(sc["cones"], sc["fraction"])
    g.close()


def planted(shape, **kw):
    """a shape of prm_simplify_helpers on the device: a chain roadmap, one query along it, solved breadth-first"""
    pts, c, r, m, span, _ = shape
    g = capi.PRMRoadmap(2, ph.BOUNDS, ph.RADIUS, 64, lvs_fraction=ph.FRACTION, **kw)
    if len(r):
        g.set_spheres(np.array(c), np.array(r))
    s, t, gr = ph.chain_query(pts)
    g.setup(s, t, gr)
    g.set_roadmap(*ph.chain_roadmap(pts))
    status, off, rows = batch_of(g, [s], [t], [gr])
    assert status[0] == capi.OK and np.array_equal(bits(rows), bits(np.array(pts, dtype=np.float64)))
    return g, status, off, rows


# ------------------------------------------------------------------------------------------------ the handle's own checker

def test_is_valid_and_check_motion_rn(r2, r6):
    rng = np.random.default_rng(11)
    g1 = capi.PRMRoadmap(1, [(0.0, 10.0)], 1.0, 16, lvs_fraction=0.05, knn_k=3)            # R^1, boxes, a k-nearest handle, no roadmap
    g1.set_boxes([[2.0], [6.5]], [[3.0], [7.0]])
    _expect(capi.ERR_PLANNER_UNINITIALISED, lambda: g1.is_valid([[1.0]]))
    _expect(capi.ERR_PLANNER_UNINITIALISED, lambda: g1.check_motion([[1.0]], [[1.5]]))
    g1.setup([1.0], [9.0], 0.5)
    s1 = rn_side(1, [(0.0, 10.0)], 0.05, boxes=([[2.0], [6.5]], [[3.0], [7.0]]))
    cases = [(g1, s1, 1, [(0.0, 10.0)]), (r2[0], r2[2], 2, R2["bounds"]), (r6[0], r6[4], 6, [(0.0, 10.0)] * 6)]
    for g, side, dim, bounds in cases:
        a = rng.uniform(-0.5, 10.5, (300, dim))
        b = a + rng.normal(0.0, 1.0, (300, dim)) * rng.choice([0.01, 0.3, 2.0], (300, 1))
        valid, motion = g.is_valid(a), g.check_motion(a, b)
        assert np.array_equal(valid, [side.is_valid(p) for p in a]), dim
        assert np.array_equal(motion, [side.valid(p, q) for p, q in zip(a, b)]), dim
        assert 0 < valid.sum() < 300 and 0 < motion.sum() < 300
        assert g.is_valid(np.zeros((0, dim))).size == 0
    g1.close()


def test_is_valid_and_check_motion_so3(so3):
    g, side = so3[0], so3[4]
    rng = np.random.default_rng(12)
    a = np.array([g3.normalise(list(v)) for v in rng.normal(0.0, 1.0, (200, 4)) * [0.3, 0.3, 0.3, 0.1] + SO3["bounds"][0]])
    b = np.array([g3.normalise(list(v)) for v in a + rng.normal(0.0, 0.15, (200, 4))])
    valid, motion = g.is_valid(a), g.check_motion(a, b)
    assert np.array_equal(valid, [side.is_valid(p) for p in a])
    assert np.array_equal(motion, [side.valid(p, q) for p, q in zip(a, b)])
    assert 0 < valid.sum() < 200 and 0 < motion.sum() < 200


# ------------------------------------------------------------------------------------------------ roadmaps

def test_r2_breadth_first_and_shortest_batches_against_the_model(r2):
    g, o, side = r2
    starts, goals, radii = r2_queries()
    for weights in (None, 0):
        status, off, rows = batch_of(g, starts, goals, radii, weights)
        assert status[2] == capi.ERR_INVALID_START_STATE and status[6] == capi.ERR_NO_SOLUTION_FOUND and (status == capi.OK).sum() >= 6
        if weights is None:                                     # the raw paths are the CPU planner's own
            for q in np.nonzero(status == capi.OK)[0]:
                o.set_problem(starts[q], goals[q], radii[q])
                assert o.solve() == capi.OK and np.array_equal(bits(o.path()), bits(raw_path(off, rows, q))), q
        before = (g.roadmap(), g.batch_paths(), g.batch_results())
        total = 0
        for m in (1, 2, 3, 7):
            for span in (0, 1, 2):
                total += check_against_model(g, side, status, off, rows, m, span)
        assert total >= 6 * 12
        if weights == 0:                                        # raw_cost is the search's own label of the goal, bit for bit
            ok = status == capi.OK
            assert np.array_equal(bits(g.simplify_results()["raw_cost"][ok]), bits(g.batch_costs()[ok]))
        after = (g.roadmap(), g.batch_paths(), g.batch_results())       # nothing else changes
        for x, y in zip(before[0] + before[1], after[0] + after[1]):
            assert np.array_equal(bits(x) if x.dtype == np.float64 else x, bits(y) if y.dtype == np.float64 else y)
        assert all(np.array_equal(before[2][k], after[2][k]) for k in before[2])
        t = g.simplify_timing()
        assert t["rounds"] == 1 and len(t["phase_ms"]) == 4 and all(v >= 0.0 for v in t["phase_ms"])


def test_r2_the_hooks_matrix(r2):
    g, _, side = r2
    starts, goals, radii = r2_queries()
    status, off, rows = batch_of(g, starts, goals, radii)
    q = int(np.nonzero(status == capi.OK)[0][0])
    for m, span in ((1, 0), (2, 0), (3, 2), (7, 1)):
        check_matrix(g, side, raw_path(off, rows, q), q, m, span)
    assert g.batch_path_valid_matrix(2, 3, 0).size == 0        # a query without a path
    _expect(capi.ERR_BAD_ARG, lambda: g.batch_path_valid_matrix(len(status), 1, 0))


def test_mixed_batches_do_not_depend_on_the_chunk(r2):
    g, _, side = r2
    starts, goals, radii = r2_queries()
    status, off, rows = batch_of(g, starts, goals, radii, 0)
    ref = simplified(g, 3, 0)
    for chunk in (1, 3):
        got = simplified(g, 3, 0, chunk)
        assert g.simplify_timing()["rounds"] == -(-len(status) // chunk)
        for x, y in zip(ref[:3], got[:3]):
            assert np.array_equal(bits(x) if x.dtype == np.float64 else x, bits(y) if y.dtype == np.float64 else y)
        assert all(np.array_equal(bits(ref[3][k]) if k != "checks" else ref[3][k], bits(got[3][k]) if k != "checks" else got[3][k])
                   for k in ref[3])
    assert check_against_model(g, side, status, off, rows, 2, 2, chunk=3) >= 6


def test_r6_against_the_model(r6):
    g, starts, goals, radii, side = r6
    for weights, m, span in ((None, 3, 0), (0, 2, 2)):
        status, off, rows = batch_of(g, starts, goals, radii, weights)
        ok = [int(q) for q in np.nonzero(status == capi.OK)[0]]
        assert len(ok) >= 3
        assert check_against_model(g, side, status, off, rows, m, span, queries=ok[:3]) == 3
        check_matrix(g, side, raw_path(off, rows, ok[0]), ok[0], 2, 0)
        if weights == 0:
            okm = status == capi.OK
            assert np.array_equal(bits(g.simplify_results()["raw_cost"][okm]), bits(g.batch_costs()[okm]))


def test_so3_against_the_model(so3):
    g, starts, goals, radii, side = so3
    for weights, m, span in ((None, 1, 0), (0, 3, 2)):
        status, off, rows = batch_of(g, starts, goals, radii, weights)
        ok = [int(q) for q in np.nonzero(status == capi.OK)[0]]
        assert status[2] == capi.ERR_INVALID_START_STATE and len(ok) >= 2
        assert check_against_model(g, side, status, off, rows, m, span, queries=ok[:2]) == 2
        if weights == 0:
            okm = status == capi.OK
            assert np.array_equal(bits(g.simplify_results()["raw_cost"][okm]), bits(g.batch_costs()[okm]))
    check_matrix(g, side, raw_path(off, rows, ok[0]), ok[0], 2, 0)


# ------------------------------------------------------------------------------------------------ limit shapes on planted chains

@pytest.mark.parametrize("name", sorted(ph.limit_shapes()))
def test_limit_shapes(name):
    shape = ph.limit_shapes()[name]
    pts, c, r, m, span, what = shape
    g, status, off, rows = planted(shape)
    side = rn_side(2, ph.BOUNDS, ph.FRACTION, (c, r))
    assert check_against_model(g, side, status, off, rows, m, span) == 1
    want = check_matrix(g, side, rows, 0, m, span)
    soff, states, idx, res = simplified(g, m, span)
    model = ph.model_of_shape(shape, side.keep)
    print("%s: %s; idx %s, checks %d" % (name, what, [int(v) for v in idx], int(res["checks"][0])))
    assert [int(v) for v in idx] == model["idx"]
    if name.startswith("matrix_"):
        assert ph.matrix_bits(len(pts), m, span) == int(name.split("_")[1])
        checked = [want[u, v] for u in range(len(want)) for v in range(u + 1, len(want)) if not ph.same_edge(u, v, m)
                   and v - u <= ph.span_of(len(pts), span) * m]
        assert any(checked) and not all(checked)
    if name == "tie":
        assert [int(v) for v in idx] == [0, 1, 3]
    if name.startswith("short_"):
        assert int(res["checks"][0]) == {"short_L2_m1": 0, "short_L2_m2": 0, "short_L3_m1": 1}[name]
    g.close()


def test_corner_is_cut_only_between_waypoints():
    shapes = ph.limit_shapes()
    cost = {}
    for name in ("corner_m1", "corner_m8"):
        g, status, off, rows = planted(shapes[name])
        cost[name] = simplified(g, shapes[name][3], 0)[3]
        g.close()
    assert cost["corner_m8"]["simplified_cost"][0] < cost["corner_m1"]["simplified_cost"][0] == cost["corner_m1"]["raw_cost"][0]
    assert np.array_equal(bits(cost["corner_m8"]["raw_cost"]), bits(cost["corner_m1"]["raw_cost"]))


def test_bits_are_preserved_rn():
    pts = [[0.0, 0.0], [1.0, -0.0], [1.0, 1.2]]                # the chord p_0 -> p_2 is blocked: the chain keeps p_1
    shape = (pts, [[0.6, 0.6]], [0.3], 1, 0, "")
    g, status, off, rows = planted(shape)
    soff, states, idx, res = simplified(g, 1, 0)
    assert [int(v) for v in idx] == [0, 1, 2] and np.array_equal(bits(states), bits(np.array(pts)))
    assert bits(states[1])[1] == 0x8000000000000000
    soff, states, idx, res = simplified(g, 4, 1)               # the copied points of a subdivided path keep their bits too
    side = rn_side(2, ph.BOUNDS, ph.FRACTION, ([[0.6, 0.6]], [0.3]))
    assert check_against_model(g, side, status, off, rows, 4, 1) == 1
    g.close()


def test_bits_are_preserved_so3():
    s = g3.normalise([0.0, 0.1, 0.0, 1.0])
    m0 = [v * 1.001 for v in g3.normalise([0.0, 0.2, 0.05, 1.0])]     # not a unit quaternion: its bits must come through
    m1 = g3.normalise([0.05, 0.35, 0.05, 1.0])
    g = capi.PRMRoadmap(4, SO3_BOUNDS, 0.15, 16, lvs_fraction=0.05, space=capi.SPACE_SO3)
    g.setup(s, m1, 1e-6)
    g.set_roadmap(np.array([m0, m1]), [0, 1, 2], [1, 0])
    status, off, rows = batch_of(g, [s], [m1], [1e-6])
    assert status[0] == capi.OK and np.array_equal(bits(rows), bits(np.array([s, m0, m1])))
    soff, states, idx, res = simplified(g, 1, 1)               # max_span 1, m 1: the path as it is
    assert [int(v) for v in idx] == [0, 1, 2] and np.array_equal(bits(states), bits(rows))
    side = so3_side([], 0.05)
    assert check_against_model(g, side, status, off, rows, 2, 0) == 1
    assert check_against_model(g, side, status, off, rows, 3, 1) == 1
    g.close()


def test_moved_obstacles_are_read_by_the_next_simplify():
    shape = ph.limit_shapes()["short_L3_m1"]
    pts = shape[0]
    g, status, off, rows = planted((pts, [], [], 1, 0, ""))
    assert [int(v) for v in simplified(g, 1, 0)[2]] == [0, 2]
    g.set_spheres(np.array(shape[1]), np.array(shape[2]))       # the same batch, a sphere across the chord: no new solve
    soff, states, idx, res = simplified(g, 1, 0)
    assert [int(v) for v in idx] == [0, 1, 2] and np.array_equal(bits(states), bits(rows))
    side = rn_side(2, ph.BOUNDS, ph.FRACTION, (shape[1], shape[2]))
    assert check_against_model(g, side, status, off, rows, 5, 0) == 1
    g.close()


# ------------------------------------------------------------------------------------------------ lifecycle

def test_lifecycle_statuses():
    shape = ph.limit_shapes()["matrix_63"]
    pts = shape[0]
    s, t, gr = ph.chain_query(pts)
    g = capi.PRMRoadmap(2, ph.BOUNDS, ph.RADIUS, 64, lvs_fraction=ph.FRACTION)
    getters = (g.simplified_batch_paths, g.simplify_results)
    for call in (g.simplify_batch_paths,) + getters + (lambda: g.batch_path_valid_matrix(0), g.simplify_timing):
        _expect(capi.ERR_PLANNER_UNINITIALISED, call)
    g.setup(s, t, gr)
    assert g.simplify_timing()["rounds"] == 0
    for call in (g.simplify_batch_paths,) + getters + (lambda: g.batch_path_valid_matrix(0),):
        _expect(capi.ERR_UNSAMPLED_STATE_SPACE, call)          # no batch yet
    g.set_roadmap(*ph.chain_roadmap(pts))

    def fresh():
        assert batch_of(g, [s], [t], [gr])[0][0] == capi.OK
        for call in getters:
            assert "no simplified paths" in _expect(capi.ERR_BAD_ARG, call)      # a batch, no simplify since it
        g.simplify_batch_paths(2, 0)
        assert len(g.simplified_batch_paths()[2]) >= 2

    fresh()
    for bad in (0, 257):
        _expect(capi.ERR_BAD_ARG, lambda: g.simplify_batch_paths(bad))
        _expect(capi.ERR_BAD_ARG, lambda: g.batch_path_valid_matrix(0, bad))
    assert len(g.simplified_batch_paths()[2]) >= 2             # a refused simplify leaves the last results as they were
    g.simplify_batch_paths(256, 1)
    fresh()
    g.set_spheres(np.array([[5.0, 9.0]]), np.array([0.1]))      # the obstacles do not drop the results
    assert len(g.simplified_batch_paths()[2]) >= 2
    changes = (lambda: g.set_roadmap(*ph.chain_roadmap(pts)), g.revalidate, lambda: g.grow(2, new_stream=5),
               lambda: g.prune(largest=True), lambda: g.setup(s, t, gr))
    for change in changes:
        change()
        for call in (g.simplify_batch_paths,) + getters:
            _expect(capi.ERR_UNSAMPLED_STATE_SPACE, call)      # the batch went with the roadmap it was solved on
        if g.sizes()[0] == 0:
            g.set_roadmap(*ph.chain_roadmap(pts))
        fresh()
    # construct_roadmap: on a roadmap that exists it is the reference's "already constructed" and changes nothing, so the results
    # stay; where it builds (after setup(), the only way to an empty roadmap under a batch) the batch and its shortcut are gone
    g.construct_roadmap()
    assert len(g.simplified_batch_paths()[2]) >= 2 and np.array_equal(bits(g.roadmap()[0]), bits(ph.chain_roadmap(pts)[0]))
    g.setup(s, t, gr)
    g.construct_roadmap()
    assert g.sizes()[0] == 64
    for call in (g.simplify_batch_paths,) + getters:
        _expect(capi.ERR_UNSAMPLED_STATE_SPACE, call)
    g.solve_batch([s], [t], [gr])
    for call in getters:
        assert "no simplified paths" in _expect(capi.ERR_BAD_ARG, call)
    g.simplify_batch_paths(2, 0)
    assert len(g.simplified_batch_paths()[0]) == 2
    g.set_roadmap(*ph.chain_roadmap(pts))
    fresh()
    g.close()


def test_null_pointers_on_a_live_handle_are_bad_arg():
    import ctypes as C
    shape = ph.limit_shapes()["short_L3_m1"]
    g, status, off, rows = planted(shape)
    g.simplify_batch_paths(2, 0)
    before = [int(v) for v in g.simplified_batch_paths()[2]]
    L, h = capi.lib(), g._h
    d, u8, n = (C.c_double * 8)(1.0, 1.0, 2.0, 0.0), (C.c_uint8 * 16)(), C.c_uint32(7)
    assert L.oxhip_prm_is_valid(h, None, 1, u8) == capi.ERR_BAD_ARG
    assert L.oxhip_prm_is_valid(h, d, 1, None) == capi.ERR_BAD_ARG
    assert L.oxhip_prm_check_motion(h, None, d, 1, u8) == capi.ERR_BAD_ARG
    assert L.oxhip_prm_check_motion(h, d, None, 1, u8) == capi.ERR_BAD_ARG
    assert L.oxhip_prm_check_motion(h, d, d, 1, None) == capi.ERR_BAD_ARG
    assert b"null" in L.oxhip_last_error_string()
    assert L.oxhip_prm_batch_path_valid_matrix(h, 0, 1, 0, u8, 16, None) == capi.ERR_BAD_ARG
    assert b"null" in L.oxhip_last_error_string()
    # the getters' pointers may each be NULL; a NULL matrix only asks for M
    assert L.oxhip_prm_batch_get_simplified_paths(h, None, None, None, 0, None) == capi.OK
    assert L.oxhip_prm_batch_get_simplify_results(h, None, None, None) == capi.OK
    assert L.oxhip_prm_batch_simplify_last_timing(h, None, None) == capi.OK
    assert L.oxhip_prm_batch_path_valid_matrix(h, 0, 2, 0, None, 0, C.byref(n)) == capi.OK and n.value == 5
    assert L.oxhip_prm_batch_path_valid_matrix(h, 0, 2, 0, u8, 16, C.byref(n)) == capi.ERR_CAPACITY and n.value == 5
    assert [int(v) for v in g.simplified_batch_paths()[2]] == before and before[0] == 0 and before[-1] == 4   # none of it touched the results
    g.close()


def test_a_path_too_large_for_one_round_is_refused():
    """400 milestones in a chain, 256 parts per edge, no max_span: (W - 1) M is beyond the 2^33 bits of 1 GiB"""
    n = 400
    pts = [[-1.9 + 0.006 * k, 0.0] for k in range(n + 1)]
    g = capi.PRMRoadmap(2, ph.BOUNDS, 0.009, n, lvs_fraction=ph.FRACTION)
    s, t, gr = ph.chain_query(pts)
    g.setup(s, t, gr)
    g.set_roadmap(*ph.chain_roadmap(pts))
    assert g.solve_batch([s], [t], [gr])[0] == capi.OK
    assert ph.matrix_bits(n + 1, 256, 0) > 2 ** 33 > ph.matrix_bits(n + 1, 256, 1)
    assert "max_span" in _expect(capi.ERR_CAPACITY, lambda: g.simplify_batch_paths(256, 0))
    assert "no simplified paths" in _expect(capi.ERR_BAD_ARG, g.simplify_results)
    g.simplify_batch_paths(256, 1)                             # a max_span makes it fit
    res = g.simplify_results()
    assert int(res["checks"][0]) == ph.expected_checks(n + 1, 256, 1) and res["simplified_cost"][0] <= res["raw_cost"][0]
    idx = g.simplified_batch_paths()[2].astype(np.int64)
    assert idx[0] == 0 and idx[-1] == n * 256 and np.all(np.diff(idx) >= 1) and np.all(np.diff(idx) <= 256)   # no link beyond the window
    g.close()


# ------------------------------------------------------------------------------------------------ the Python planner

def _goal(target, radius):
    class Goal:
        pass
    goal = Goal()
    goal.target, goal.radius = target, radius
    return goal


def test_python_planner_r2():
    from oxmpl_amd.base import Path, ProblemDefinition, RealVectorState, RealVectorStateSpace, SphereBoxValidityChecker
    from oxmpl_amd.geometric import PRM
    space = RealVectorStateSpace(2, R2["bounds"])
    space.longest_valid_segment_fraction = R2["fraction"]
    starts, goals, radii = r2_queries()
    pds = [ProblemDefinition(space, RealVectorState(list(s)), _goal(RealVectorState(list(t)), float(r))) for s, t, r in zip(starts, goals, radii)]
    p = PRM(1.0, R2["radius"], pds[0], max_milestones=R2["n"], seed=R2["seed"], stream=R2["stream"])
    p.setup(SphereBoxValidityChecker(spheres=[(list(c), float(r)) for c, r in zip(*R2["spheres"])]))
    p.construct_roadmap()
    with pytest.raises(Exception) as ei:
        p.simplify_batch()
    assert "not sampled" in str(ei.value)
    raw = p.solve_batch(pds, 1.0, shortest=True)
    simp = p.simplify_batch(subdivide=4)
    assert len(simp) == len(raw)
    side = rn_side(2, R2["bounds"], R2["fraction"], R2["spheres"])
    for a, b in zip(raw, simp):
        assert (b is None) == isinstance(a, Exception)
        if b is None:
            continue
        assert isinstance(b, Path) and b.states[0].values == a.states[0].values and b.states[-1].values == a.states[-1].values
        rows = [s.values for s in b.states]
        assert all(side.valid(u, v) for u, v in zip(rows, rows[1:]))
        length = lambda path: sum(orc.distance(u.values, v.values) for u, v in zip(path.states, path.states[1:]))  # noqa: E731
        assert length(b) <= length(a) * (1.0 + 1e-12)
    with pytest.raises(ValueError):
        p.simplify_batch(subdivide=0)
    one = p.simplify_solution(subdivide=4, max_span=0)         # the planner's own query, as a one-query batch
    assert one.states[0].values == list(starts[0]) and len(p.simplify_batch(4)) == 1
    p.set_problem_definition(pds[2])                           # a start in collision
    with pytest.raises(Exception) as ei:
        p.simplify_solution()
    assert "Start state is not valid" in str(ei.value)


def test_python_planner_so3():
    from oxmpl_amd.base import ProblemDefinition, SO3ConeValidityChecker, SO3State, SO3StateSpace
    from oxmpl_amd.geometric import PRM
    sc = SO3
    space = SO3StateSpace((SO3State(*sc["bounds"][0]), sc["bounds"][1]))
    s, t, gr = sc["queries"][0]
    pd = ProblemDefinition(space, SO3State(*s), _goal(SO3State(*t), gr))
    p = PRM(1.0, sc["radius"], pd, max_milestones=300, seed=sc["seed"], stream=sc["stream"])
    p.setup(SO3ConeValidityChecker(cones=[(SO3State(*c), r) for c, r in sc["cones"]]))
    p.construct_roadmap()
    raw = p.solve(1.0)
    one = p.simplify_solution(subdivide=3)
    side = so3_side(sc["cones"], sc["fraction"])
    rows = [st.values for st in one.states]
    assert rows[0] == raw.states[0].values and rows[-1] == raw.states[-1].values and 2 <= len(rows)
    assert all(side.valid(u, v) for u, v in zip(rows, rows[1:]))
    assert sum(side.dist(u, v) for u, v in zip(rows, rows[1:])) <= sum(side.dist(u.values, v.values) for u, v in zip(raw.states, raw.states[1:])) * (1 + 1e-12)
