"""CPU: the limit shapes of rrt_so2.hip (tests/so2_limits_shapes.py) held to their purpose on the checker
(tests/golden/make_golden_so2.py).  Per shape it prints the step count, the index of the first invalid state, and the winning
node with its rivals; a shape that no longer hits its target fails here instead of passing silently on the GPU."""
import pytest

import so2_helpers as h
import so2_limits_shapes as shapes
from so2_helpers import so2

PLANNER = shapes.planner_shapes()


def test_the_shapes_follow_the_kernel_constants():
    assert (shapes.K, shapes.KA) == h.kernel_constants()
    assert {"mirror_%d" % n for n in (shapes.K - 1, shapes.K, shapes.K + 1, shapes.K + 65)} <= set(PLANNER)
    assert {"arcs_%d_blocked" % n for n in (1, shapes.KA, shapes.KA + 1)} <= set(PLANNER) and "arcs_0_open" in PLANNER


@pytest.mark.parametrize("name", sorted(PLANNER))
def test_planner_shape_hits_its_target(name):
    shape = PLANNER[name]
    sc, ex = shape["sc"], shape["expect"]
    trace = []
    res = shapes.run(shape, trace)
    states = shape.get("tree") or [sc["start"]]
    print(name, "n", res["n"], "iterations", res["iterations"], "accepted", res["accepted"], "draws", res["rng_draws"])
    for it, want in enumerate(ex.get("nearest", [])):
        q, nearest, min_dist, q_new, ok = trace[it]
        rivals = [(i, so2.distance(states[i], q)) for i in ex.get("rivals", [])]
        print("  iteration", it, "query", q, "winner", nearest, min_dist, "rivals", rivals)
        assert nearest == want
        if name.startswith("tie"):
            assert rivals and all(d == min_dist for _, d in rivals)          # exact ties: the index decides
        elif name.startswith("seam"):
            assert all(d > min_dist and abs(states[i] - q) < abs(states[nearest] - q) for i, d in rivals)   # |a - b| alone errs
        elif name.startswith("antipodal"):
            assert so2.distance(states[0], q) == so2.PI and all(d >= min_dist for _, d in rivals)
    if name.startswith("mirror"):
        n = len(states)
        assert res["n"] > n and len(ex["nearest"]) == (2 if n <= shapes.K else 3 if n == shapes.K + 1 else 4)
        assert any(t[1] >= n for t in trace)                                 # later samples find the nodes the run itself added
    if "blocked" in ex:
        assert len(sc["arcs"]) == ex["n_arcs"]
        assert (res["goal_node"] < 0 and 0 < res["accepted"] < res["iterations"]) if ex["blocked"] else res["goal_node"] > 0
        if ex["blocked"]:   # the last arc decides: without it the same run reaches the goal
            assert shapes.run(dict(shape, sc=dict(sc, arcs=sc["arcs"][:-1])))["goal_node"] > 0
    if "steps" in ex:
        sts = so2.motion_states(sc["fraction"], sc["start"], sc["target"])
        bad = [i for i, v in enumerate(sts) if not so2.Arcs(sc["arcs"]).is_valid(v)]
        print("  steps", len(sts), "invalid states", bad)
        assert len(sts) == ex["steps"] and bad == ([] if ex["first_bad"] is None else [ex["first_bad"]])
        assert res["accepted"] == ex["accepted"] and trace[0][1] == 0 and trace[0][3] == sc["target"]
    if ex.get("redraws"):
        print("  words per iteration", res["rng_draws"] / res["iterations"])
        assert res["rng_draws"] > 2 * res["iterations"] + 20    # rejected range draws: more than two words per iteration
    if "draws" in ex:
        assert res["rng_draws"] == ex["draws"]
    if "n" in ex:
        assert res["n"] == ex["n"] and res["iterations"] == ex["iterations"] and ex["iterations"] % 64 != 0


def test_validity_rows_hit_the_closed_ends_and_the_seam():
    arcs, rows = shapes.validity_rows()
    ck = so2.Arcs(arcs)
    for v, want in rows:
        print(v, so2.normalise(v), ck.is_valid(v))
        assert ck.is_valid(v) == want, v
    assert any(lo < -so2.PI < hi for lo, hi in arcs)
    assert sum(1 for v, _ in rows if any(so2.normalise(v) in arc for arc in arcs)) >= 6   # states exactly on an end


def test_motion_rows_hit_every_pass_boundary():
    seen = set()
    for arcs, frm, to, n, first_bad in shapes.motion_rows():
        sts = so2.motion_states(0.05, frm, to)
        bad = [i for i, v in enumerate(sts) if not so2.Arcs(arcs).is_valid(v)]
        print("steps", len(sts), "dist / res", so2.distance(frm, to) / shapes.RES, "invalid", bad)
        assert len(sts) == n and bad == ([] if first_bad is None else [first_bad])
        assert so2.check_motion(so2.Arcs(arcs), 0.05, frm, to) == (first_bad is None)
        seen.add((n, first_bad))
    for n in (1, 2, 64, 65, 128, 129):
        assert (n, n - 1) in seen and (n, None) in seen
    assert {(65, 64), (128, 64), (129, 64), (2, 0), (3, 0)} <= seen   # state 65; the step counts beside dist / res = 1 and 2
