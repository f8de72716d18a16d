"""The shortcut's two entries on one planted path (shortcut_core.hip, DESIGN.md sections 18 and 25): the waypoint case of the dense
shortcut is m = 1, so the RRT route -- plant a tree, set_tree, extract_paths, simplify_paths(max_span) -- and the PRM route -- a chain
roadmap, one query along it, solve_batch, simplify_batch_paths(1, max_span) -- run the same kernels over the same rows and must
return the same indices, rows, raw_cost, simplified_cost, checks and verdict matrix, bit for bit; and both must equal the two Python
models (prm_simplify_helpers.dense_shortcut, simplify_helpers.shortcut_dp) over the CPU side's check_motion, distance and interpolate.

Cases: the m = 1 limit shapes of prm_simplify_helpers in R^2, each at its own span and at max_span = 2; five states in R^8 (the pair
kernel's instantiation with the most SGPR spills) and six quaternions in SO(3), both verdicts among their chords; and a batch of four
paths of lengths 2, 0, 9, 3 run in rounds of 1, 2 and all, so that a round's tables begin at a problem / query other than the first,
with an unsolved problem / unanswered query in the middle.  What every case is claimed to hold is checked on the CPU first
(test_cases_are_held_to_their_purpose needs no GPU)."""
import math
import os
import sys

import numpy as np
import pytest

from oxmpl_amd import capi
from oracle import oracle_py as orc
from helpers import bits
import prm_simplify_helpers as ph
import rrt_revalidate_helpers as rh
import simplify_helpers as sh
import simplify_limits_shapes as sl

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_so3 as g3  # noqa: E402

SO3_BOUNDS = [0.0, 0.0, 0.0, 1.0, math.pi]
NOWHERE = [11.0, 11.5]        # the unsolved problem's goal and the unanswered query's start: no node, no milestone near it


# ------------------------------------------------------------------------------------------------ the cases

def _case(dim, bounds, fraction, radius, obstacles, paths, span, both, so3=False, chunks=(0,)):
    """paths: one [L][dim] list per problem / query, None where it has no path.  both: chords of both verdicts lie in the window."""
    return dict(dim=dim, bounds=bounds, fraction=fraction, radius=radius, obstacles=obstacles, span=span, both=both, so3=so3, chunks=chunks,
                paths=[None if p is None else np.array(p, dtype=np.float64) for p in paths])


def r8_case():
    """p_k = (k, k odd, (k odd) / 2, 0, 0, 0, 0, k / 4): a sphere on the chord p_0 -> p_2 and one on p_2 -> p_4; p_0 -> p_3 passes"""
    pts = [[float(k), float(k % 2), 0.5 * (k % 2), 0.0, 0.0, 0.0, 0.0, 0.25 * k] for k in range(5)]
    centres = [[1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.25], [3.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.75]]
    return _case(8, [(-2.0, 12.0)] * 8, ph.FRACTION, 2.0, (centres, [0.2, 0.2]), [pts], 0, True)


def so3_case():
    """simplify_limits_shapes.so3_arc in small: rotations about one axis at half-angles 0.05 + 0.1 k, each nudged off the axis, every
    odd one stored as -q; a cone between nodes 1 and 2 and one between 4 and 5, so chords across them fail and 2 -> 4 passes"""
    rng = np.random.RandomState(7)
    axis = np.array([1.0, 2.0, 3.0])
    h = 0.05 + 0.1 * np.arange(6)
    q = np.zeros((6, 4))
    for k in range(6):
        v = rh.quat_mul(rh.quat_axis_half(axis, h[k]), rh.quat_axis_half(rng.normal(size=3), 0.003))
        q[k] = v / math.sqrt(float(v @ v))
    q[1::2] *= -1.0
    cones = [rh.quat_axis_half(axis, 0.5 * (h[a] + h[a + 1])) for a in (1, 4)]
    return _case(4, None, 0.1, 0.15, (cones, [0.012, 0.012]), [q], 0, True, so3=True)


def mixed_case():
    """short_L2_m1, no path, matrix_63's zigzag and short_L3_m1, four rows apart in y so that no start reaches another chain"""
    shapes = ph.limit_shapes()
    paths, centres, radii = [], [], []
    for name, dy in (("short_L2_m1", 0.0), (None, None), ("matrix_63", 4.0), ("short_L3_m1", 8.0)):
        if name is None:
            paths.append(None)
            continue
        pts, c, r = shapes[name][:3]
        paths.append([[x, y + dy] for x, y in pts])
        centres += [[x, y + dy] for x, y in c]
        radii += list(r)
    return _case(2, ph.BOUNDS, ph.FRACTION, ph.RADIUS, (centres, radii), paths, 0, True, chunks=(1, 2, 0))


def cases():
    shapes = ph.limit_shapes()
    out = {}
    for name in ("matrix_63", "corner_m1", "tie", "short_L2_m1", "short_L3_m1"):
        pts, c, r, m, span, _ = shapes[name]
        assert m == 1 and span == 0
        for s in (0, 2):
            out["%s_span%d" % (name, s)] = _case(2, ph.BOUNDS, ph.FRACTION, ph.RADIUS, (c, r), [pts], s, name == "matrix_63" and s == 0)   # (the zigzag's skip-one chords all fail)
    out["r8"] = r8_case()
    out["so3"] = so3_case()
    out["mixed"] = mixed_case()
    out["mixed_span2"] = dict(mixed_case(), span=2, both=False)
    return out


CASES = cases()
assert [len(p) for p in CASES["matrix_63_span0"]["paths"]] == [9]
assert [0 if p is None else len(p) for p in CASES["mixed"]["paths"]] == [2, 0, 9, 3]


class Side:
    """the CPU side of a case: valid(a, b), dist(a, b), interp(a, b, t)"""

    def __init__(self, case):
        c, r = case["obstacles"]
        if case["so3"]:
            cones = g3.Cones(list(zip([list(x) for x in c], r)))
            self.valid = lambda a, b: bool(g3.check_motion(cones, case["fraction"], list(a), list(b)))
            self.dist = lambda a, b: g3.distance(list(a), list(b))
            self.interp = lambda a, b, t: g3.interpolate(list(a), list(b), t)
            return
        dim = case["dim"]
        self.o = orc.OracleRRT(dim, case["bounds"], 0.5, 0.0, case["fraction"], 16, True, 1, 0)
        if len(r):
            self.o.set_spheres(np.array(c, dtype=np.float64).reshape(-1, dim), np.array(r, dtype=np.float64))
        self.o.setup([-1.0] * dim, [11.0] * dim, 0.1)
        self.valid = lambda a, b: bool(self.o.check_motion(a, b))
        self.dist, self.interp = orc.distance, orc.interpolate


def models(case, side, pts):
    """(idx, raw, simp, checks) of one path by both Python models, which must agree before either is a yardstick"""
    if pts is None:
        return [], 0.0, 0.0, 0
    d = ph.dense_shortcut(list(pts), 1, case["span"], side.valid, side.dist, side.interp)
    w = sh.shortcut_dp(len(pts), lambda i, j: side.valid(pts[i], pts[j]), lambda i, j: side.dist(pts[i], pts[j]), case["span"])
    assert (d["idx"], bits(np.float64(d["raw"])), bits(np.float64(d["simp"])), d["checks"]) == (w[0], bits(np.float64(w[1])), bits(np.float64(w[2])), w[3])
    assert np.array_equal(bits(np.array(d["dense"])), bits(pts))           # m = 1: the dense path is the path
    return w


def window_verdicts(case, side, pts):
    """the CPU verdict of every chord (i, j), 2 <= j - i <= span"""
    L = len(pts)
    S = ph.span_of(L, case["span"])
    return {(i, j): side.valid(pts[i], pts[j]) for i in range(L) for j in range(i + 2, min(L, i + S + 1))}


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_are_held_to_their_purpose(name):
    case = CASES[name]
    side = Side(case)
    milestones = [(q, k, p) for q, pts in enumerate(case["paths"]) if pts is not None for k, p in enumerate(pts) if k >= 1]
    seen = set()
    for q, pts in enumerate(case["paths"]):
        if pts is None:
            assert all(side.dist(NOWHERE, p) > 2.0 * case["radius"] for _, _, p in milestones)
            continue
        # the query's start connects to its own p_1 alone (prm.rs: distance < radius, then check_motion), so the answer is the chain
        near = [(r, k) for r, k, p in milestones if side.dist(pts[0], p) < case["radius"]]
        assert near == [(q, 1)] and side.valid(pts[0], pts[1]), (name, q, near)
        assert all(side.dist(pts[0], p) >= case["radius"] for p in pts[2:])
        seen.update(window_verdicts(case, side, pts).values())
        models(case, side, pts)
    if case["both"]:
        assert seen == {True, False}, (name, seen)


# ------------------------------------------------------------------------------------------------ the two routes

def rrt_route(case):
    """the case's paths planted as trees -> the batch, its paths extracted"""
    paths, so3 = case["paths"], case["so3"]
    probs = []
    for p, pts in enumerate(paths):
        if pts is None:
            probs.append(sl.plant(np.array([[10.0, 9.0], [10.5, 9.5], [11.0, 9.0]]), 3, 40 + p, unsolved_goal=NOWHERE))
        else:
            probs.append(sl.plant(pts, 3, 20 + p, so3=so3))
    max_nodes = max(len(parents) for _, parents, _, _ in probs) + 8
    if so3:
        g = capi.RRTBatch(4, SO3_BOUNDS, 0.3, 0.05, len(probs), max_nodes, case["fraction"], False, 7, space=capi.SPACE_SO3)
    else:
        g = capi.RRTBatch(case["dim"], case["bounds"], 0.5, 0.05, len(probs), max_nodes, case["fraction"], False, 7)
    g.setup(np.array([s[0] for s, _, _, _ in probs]), np.array([goal[0] for _, _, goal, _ in probs]), np.array([goal[1] for _, _, goal, _ in probs]))
    for p, (states, parents, _, _) in enumerate(probs):
        g.set_tree(p, states, parents)
    r = g.revalidate_trees()                                   # no obstacle yet: nothing goes, the goal nodes are found from the states
    assert not r["n_removed"].any() and not r["goal_lost"].any()
    assert g.counts()["goal_node"].tolist() == [node for _, _, _, node in probs]
    if len(case["obstacles"][1]):
        g.set_spheres(*case["obstacles"])
    g.extract_paths()
    return g


def prm_route(case):
    """one chain of milestones per path, one query per path -> the roadmap handle, its batch solved breadth-first"""
    paths = case["paths"]
    ms, nbrs, off = [], [], [0]
    for pts in paths:
        if pts is None:
            continue
        first, n = len(ms), len(pts) - 1
        ms += [list(p) for p in pts[1:]]
        for i in range(n):
            nbrs += [first + j for j in (i - 1, i + 1) if 0 <= j < n]
            off.append(len(nbrs))
    kw = dict(space=capi.SPACE_SO3) if case["so3"] else {}
    g = capi.PRMRoadmap(case["dim"], SO3_BOUNDS if case["so3"] else case["bounds"], case["radius"], 64, lvs_fraction=case["fraction"], **kw)
    if len(case["obstacles"][1]):
        g.set_spheres(*case["obstacles"])
    solved = [pts for pts in paths if pts is not None]
    g.setup(list(solved[0][0]), list(solved[0][-1]), 1e-6)
    g.set_roadmap(np.array(ms, dtype=np.float64), np.array(off, dtype=np.uint64), np.array(nbrs, dtype=np.uint32))
    starts = [NOWHERE if pts is None else list(pts[0]) for pts in paths]
    goals = [NOWHERE if pts is None else list(pts[-1]) for pts in paths]
    status = g.solve_batch(starts, goals, [1e-6] * len(paths)).copy()
    assert (status == capi.OK).tolist() == [pts is not None for pts in paths], status
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_both_entries_return_the_same_bits_and_the_models(name):
    case = CASES[name]
    side = Side(case)
    span, paths = case["span"], case["paths"]
    lengths = [0 if pts is None else len(pts) for pts in paths]
    want = [models(case, side, pts) for pts in paths]
    r, p = rrt_route(case), prm_route(case)
    # both routes hold the planted paths, row for row
    roff, rrows = r.paths()
    poff, _, prows = p.batch_paths()
    assert np.diff(roff.astype(np.int64)).tolist() == lengths and np.diff(poff.astype(np.int64)).tolist() == lengths, name
    planted = np.concatenate([pts for pts in paths if pts is not None])
    assert np.array_equal(bits(rrows), bits(planted)) and np.array_equal(bits(prows), bits(planted))
    for chunk in case["chunks"]:
        r.simplify_paths(span, chunk)
        p.simplify_batch_paths(1, span, chunk)
        rounds = -(-len(paths) // chunk) if chunk else 1
        assert r.paths_last_timing()["rounds"] == rounds == p.simplify_timing()["rounds"]
        off_r, rows_r, idx_r, raw_r, simp_r, checks_r = r.simplified_paths()
        off_p, rows_p, idx_p = p.simplified_batch_paths()
        res = p.simplify_results()
        assert off_r.tolist() == off_p.tolist() and idx_r.tolist() == idx_p.tolist(), (name, chunk)
        assert np.array_equal(bits(rows_r), bits(rows_p)), (name, chunk)
        assert np.array_equal(bits(raw_r), bits(res["raw_cost"])) and np.array_equal(bits(simp_r), bits(res["simplified_cost"])), (name, chunk)
        assert checks_r.tolist() == res["checks"].tolist(), (name, chunk)
        for q, (pts, (idx, raw, simp, checks)) in enumerate(zip(paths, want)):
            a, b = int(off_r[q]), int(off_r[q + 1])
            assert idx_r[a:b].tolist() == idx, (name, chunk, q)
            assert bits(raw_r[q]) == bits(np.float64(raw)) and bits(simp_r[q]) == bits(np.float64(simp)), (name, chunk, q)
            assert int(checks_r[q]) == checks == ph.expected_checks(lengths[q], 1, span) == sh.expected_checks(lengths[q], span), (name, chunk, q)
            if pts is not None:
                assert np.array_equal(bits(rows_r[a:b]), bits(pts[idx])), (name, chunk, q)
    # the verdict matrices: the two hooks agree, and every chord of the window is the CPU's verdict
    for q, pts in enumerate(paths):
        mr, mp = r.path_valid_matrix(q, span), p.batch_path_valid_matrix(q, 1, span)
        if pts is None:
            assert mr.size == 0 and mp.size == 0
            continue
        L = len(pts)
        assert mr.shape == mp.shape == (L, L) and np.array_equal(mr, mp), (name, q)
        cpu = np.zeros((L, L), dtype=bool)
        cpu[np.arange(L - 1), np.arange(1, L)] = True                      # the planner's edges: true without a check
        for (i, j), ok in window_verdicts(case, side, pts).items():
            cpu[i, j] = ok
        assert np.array_equal(mr, cpu), (name, q)
    r.close()
    p.close()
