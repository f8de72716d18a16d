"""The limit shapes of rrt_so2.hip, shared by tests/test_so2_limits_model.py (CPU: every shape still hits its target on the
checker) and tests/test_gpu_so2_limits.py (GPU: the kernel equals the checker on every shape).  Nothing here touches the library.

A planner shape is a dict: sc (a scene of so2_helpers.scene), seed, pid, iterations, optionally tree / parents (planted with
set_tree after setup) and cuts (the solve calls the budget is cut into), and `expect`: what the checker's trace must show for
the shape to serve its purpose -- nearest indices of the first iterations, verdicts, counts."""
import numpy as np

import so2_helpers as h
from so2_helpers import so2

PI = so2.PI
K, KA = h.K_SO2_N, h.K_SO2_LDS_ARCS
RES = PI * 0.05 * 0.1   # check_motion's step at fraction 0.05


def samples(seed, pid, bounds, count):
    """the first `count` uniform samples of a problem with goal_bias 0 (a Bernoulli word, then the range draw, per iteration)"""
    rng = so2.mg.ChaCha12Rng(seed, pid)
    lo, hi = so2.space_bounds(bounds)
    out = []
    for _ in range(count):
        assert not so2.mg.random_bool(rng, 0.0)
        out.append(so2.mg.random_range(rng, lo, hi))
    return out


def run(shape, trace=None):
    sc = shape["sc"]
    return so2.rrt_solve(sc["bounds"], sc["max_distance"], sc["goal_bias"], sc["fraction"], so2.Arcs(sc["arcs"]), sc["start"],
                         sc["target"], sc["goal_r"], shape["seed"], shape["pid"], shape["iterations"], sc["max_nodes"],
                         stop_at_goal=shape.get("stop_at_goal", True), tree=shape.get("tree"), parents=shape.get("parents"), trace=trace)


# ------------------------------------------------------------------------------------------------ the LDS mirror
def mirror_shapes():
    """planted trees of K - 1, K, K + 1 and K + 65 nodes, then 64 iterations: the first samples find their nearest node at index
    0, K - 1, K and the last index (those the planted tree has): a node 1e-3 beside the sample, the rest of the tree far away"""
    out = {}
    for n in (K - 1, K, K + 1, K + 65):
        seed, pid, bounds = 11, n, (-1.0, 1.0)
        q = samples(seed, pid, bounds, 4)
        states = np.linspace(2.0, 2.5, n).tolist()   # far from every sample
        marks = [i for i in (0, K - 1, K, n - 1) if i < n]
        marks = sorted(set(marks))
        for qi, i in zip(q, marks):
            states[i] = qi + 1e-3
        sc = h.scene(bounds=bounds, max_distance=0.01, goal_bias=0.0, start=states[0], target=-3.0, goal_r=0.01, arcs=[(1.2, 1.3)],
                     max_nodes=n + 100)
        out["mirror_%d" % n] = dict(sc=sc, seed=seed, pid=pid, iterations=64, tree=states, parents=[-1] + [0] * (n - 1),
                                    expect=dict(nearest=marks))
    return out


# ------------------------------------------------------------------------------------------------ ties, the seam, antipodes
def _query_shape(nodes, target, nearest, rivals=(), iterations=2, max_distance=0.05, arcs=()):
    """goal_bias 1: every sample is the target, no word is drawn -- the query is ours to place"""
    sc = h.scene(max_distance=max_distance, goal_bias=1.0, start=nodes[0], target=target, goal_r=1e-9, arcs=arcs, max_nodes=len(nodes) + 10)
    return dict(sc=sc, seed=1, pid=0, iterations=iterations, tree=list(nodes), parents=[-1] + [0] * (len(nodes) - 1),
                expect=dict(nearest=[nearest], rivals=list(rivals)))


def tie_shapes():
    far = np.linspace(2.0, 2.5, 80).tolist()
    out = {}
    t = list(far)
    t[5], t[9] = 0.75, 0.25                       # q + d and q - d, d = 0.25: both distances are 0.25 exactly
    out["tie_plus_minus"] = _query_shape(t, 0.5, 5, rivals=[9])
    t = list(far)
    t[9], t[5] = 0.75, 0.25
    out["tie_minus_plus"] = _query_shape(t, 0.5, 5, rivals=[9])
    t = list(far)
    t[3] = t[67] = t[70] = 0.75                   # exact duplicates: the same lane's next stride (67 = 3 + 64) and another lane
    out["tie_duplicates"] = _query_shape(t, 0.5, 3, rivals=[67, 70])
    t = list(far)
    t[70] = t[3 + 64] = 0.25
    t[12] = 0.75                                  # the lowest index among three lanes' candidates
    out["tie_across_lanes"] = _query_shape(t, 0.5, 12, rivals=[67, 70])
    # the seam: the nearest node lies on the other side of +-PI (|a - b| alone would choose the rival)
    out["seam_from_below"] = _query_shape([0.0, PI - 0.01, -PI + 0.7], -PI + 0.3, 1, rivals=[2])
    out["seam_from_above"] = _query_shape([0.0, PI - 0.7, -PI + 0.01], PI - 0.3, 2, rivals=[1])
    # a query exactly antipodal to a node: distance PI, whichever way round; alone, and with a rival a hair nearer
    out["antipodal_alone"] = _query_shape([0.5 - PI], 0.5, 0, max_distance=0.2)
    out["antipodal_rival"] = _query_shape([0.5 - PI, 0.5 - PI + 1e-9, 0.5 - PI], 0.5, 1, rivals=[0, 2], max_distance=0.2)
    return out


# ------------------------------------------------------------------------------------------------ arcs
def _slivers(count):
    return [(2.0 + 0.01 * j, 2.0 + 0.01 * j + 0.001) for j in range(count)]   # far from the states under test


def arc_shapes():
    """0, 1, KA and KA + 1 arcs with the deciding arc last: the target lies in the last arc alone, so every motion is rejected --
    and accepted once that arc is taken away (the `open` twin)"""
    out = {}
    for count in (0, 1, KA, KA + 1):
        for last in (True, False):
            if count == 0 and last:
                continue
            arcs = _slivers(count - 1 if last else count) + ([(0.55, 0.65)] if last else [])
            sc = h.scene(max_distance=0.05, goal_bias=1.0, start=0.0, target=0.6, goal_r=1e-9, arcs=arcs, max_nodes=100)
            out["arcs_%d_%s" % (count, "blocked" if last else "open")] = dict(
                sc=sc, seed=2, pid=count, iterations=14, expect=dict(blocked=last, n_arcs=count))
    return out


def validity_rows():
    """(arcs, states, expected verdicts): the closed ends, and an arc that contains -PI"""
    v = so2.normalise(7.0)          # an arc end exactly equal to a state's normalised value
    w = so2.normalise(-8.5)
    arcs = [(v, 1.0), (-2.5, w), (-3.5, -3.0)]
    nx = lambda x, d: x + d * 1e-9  # noqa: E731  (a neighbour in binary64 can normalise onto the end itself: v + PI absorbs an ulp)
    rows = [(7.0, False), (v, False), (nx(v, -1.0), True), (1.0, False), (nx(1.0, 1.0), True), (-8.5, False), (w, False),
            (nx(w, 1.0), True), (-2.5, False), (nx(-2.5, -1.0), True),
            (PI, False), (-PI, False), (3.1, True), (-3.1, False), (-3.0, False), (nx(-3.0, 1.0), True), (3.0, True), (3.2, False)]
    return arcs, rows


# ------------------------------------------------------------------------------------------------ motion passes
def motion_rows():
    """check_motion rows of N = 1, 2, 64, 65, 128, 129 states from 0 to (N - 0.5) res.  Per row: (arcs, from, to, N, first invalid
    state or None).  The only invalid state is the last one, or state 65 (index 64); the `clear` twin's arc lies just past the end."""
    rows = []
    for N in (1, 2, 64, 65, 128, 129):
        to = (N - 0.5) * RES
        states = so2.motion_states(0.05, 0.0, to)
        last = states[-1]
        rows.append(([(last - RES / 4, last + RES / 4)], 0.0, to, N, N - 1))
        rows.append(([(to + RES / 4, to + RES / 2)], 0.0, to, N, None))
        if N >= 65:
            rows.append(([(states[64] - RES / 4, states[64] + RES / 4)], 0.0, to, N, 64))
    # dist / res just either side of 1 and 2: an arc on a state that only the larger step count tests (to / 2 resp. to / 3)
    for mult, n, probe in ((1.0 - 1e-12, 1, 0.5), (1.0 + 1e-12, 2, 0.5), (2.0 * (1.0 - 1e-12), 2, 1.0 / 3.0), (2.0 * (1.0 + 1e-12), 3, 1.0 / 3.0)):
        to = RES * mult
        at = to * probe
        rows.append(([(at - RES / 8, at + RES / 8)], 0.0, to, n, 0 if n * probe > 0.9 else None))
    return rows


def motion_planner_shapes():
    """the same motions as planner steps: max_distance 4, goal_bias 1, so the first motion runs from the start to the target"""
    out = {}
    for arcs, frm, to, N, first_bad in motion_rows():
        sc = h.scene(max_distance=4.0, goal_bias=1.0, start=frm, target=to, goal_r=1e-9, arcs=arcs, max_nodes=50)
        name = "motion_%d_%s_%d" % (N, "clear" if first_bad is None else "bad%d" % first_bad, len(out))
        out[name] = dict(sc=sc, seed=3, pid=N, iterations=3, expect=dict(accepted=1 if first_bad is None else 0, steps=N, first_bad=first_bad))
    return out


# ------------------------------------------------------------------------------------------------ sampler and stops
def sampler_shapes():
    lo = 1.0
    hi = float(np.nextafter(np.nextafter(np.nextafter(lo, 2.0), 2.0), 2.0))   # three ulps: a third of the draws round up to hi
    tight = h.scene(bounds=(lo, hi), max_distance=0.2, goal_bias=0.05, start=lo, target=lo, goal_r=0.0, arcs=[(2.0, 2.1)], max_nodes=1000)
    out = {"sampler_redraws": dict(sc=tight, seed=4, pid=1, iterations=200, stop_at_goal=False, cuts=[200], expect=dict(redraws=True)),
           "sampler_redraws_cut": dict(sc=tight, seed=4, pid=1, iterations=200, stop_at_goal=False, cuts=[100, 30, 70], expect=dict(redraws=True))}
    fx = so2.fixture_scene()
    out["bias0"] = dict(sc=dict(fx, goal_bias=0.0, max_nodes=500), seed=4, pid=2, iterations=150, stop_at_goal=False, cuts=[150], expect={})
    out["bias0_cut_in_block"] = dict(sc=dict(fx, goal_bias=0.0, max_nodes=500), seed=4, pid=2, iterations=150, stop_at_goal=False,
                                     cuts=[37, 64, 49], expect={})
    out["bias1"] = dict(sc=dict(fx, goal_bias=1.0, max_nodes=500), seed=4, pid=3, iterations=150, stop_at_goal=False, cuts=[100, 50],
                        expect=dict(draws=0))
    return out


def stop_shapes():
    free = h.scene(max_distance=0.05, goal_bias=0.05, start=0.0, target=3.0, goal_r=0.01, arcs=[], max_nodes=40)
    return {"max_nodes_mid_block": dict(sc=free, seed=6, pid=0, iterations=200, expect=dict(n=40, iterations=39))}


def planner_shapes():
    out = {}
    for part in (mirror_shapes(), tie_shapes(), arc_shapes(), motion_planner_shapes(), sampler_shapes(), stop_shapes()):
        out.update(part)
    return out
