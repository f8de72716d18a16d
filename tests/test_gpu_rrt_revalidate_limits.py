"""GPU: oxhip_rrt_batch_revalidate_trees (rrt_revalidate.hip) on the shapes of
tests/rrt_revalidate_limits_shapes.py, which tests/test_rrt_revalidate_limits_model.py holds to their properties on the CPU.

Families A .. F: every shape is planted with set_tree and compared bit for bit with the references (the C oracle over R^n,
make_golden_so3.py, make_golden_so2.py for edge verdicts and goal membership, the plain loops of rrt_revalidate_helpers.py for the
rest): tree(), the parents, revalidate_map(), n_removed, goal_lost, counts().  The batch's own check_motion on the same (parent,
node) rows must give the references' verdicts too.  No tolerance anywhere.
Family G (skip flags) and H (a handle used round after round) compare a batch re-checked on the device with a twin pruned on the
host through get_tree / check_motion / set_tree, before and after further solves.
Last: a refused call (RRTConnect, RRT*) leaves extracted paths as they were."""
import math

import numpy as np
import pytest

from oxmpl_amd import capi, scenarios

import rrt_revalidate_helpers as rh
import rrt_revalidate_limits_shapes as sh
import so2_helpers as h2

pytestmark = pytest.mark.gpu
SPACE = dict(rn=capi.SPACE_REAL_VECTOR, so3=capi.SPACE_SO3, so2=capi.SPACE_SO2)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def make_batch(S, kernel=capi.KERNEL_AUTO, goal_bias=0.05, seed=7):
    P = len(S["trees"])
    # max_distance: a twentieth of the first axis over R^n (0.5 in [0, 10]^d, and as much in every frame)
    step = 0.05 * (S["bounds"][0][1] - S["bounds"][0][0]) if S["space"] == "rn" else dict(so3=0.3, so2=0.2)[S["space"]]
    b = capi.RRTBatch(S["dim"], S["bounds"], step, goal_bias, P, S["max_nodes"], S["fraction"], False, seed, kernel=kernel,
                      space=SPACE[S["space"]])
    b.setup(np.array([s[0] for s, _ in S["trees"]]), np.array([c for c, _ in S["goals"]]), np.array([r for _, r in S["goals"]]))
    return b


def plant(b, S):
    for p, (s, par) in enumerate(S["trees"]):
        b.set_tree(p, s, par)


def set_obstacles(b, S):
    if len(S["sph_r"]):
        b.set_spheres(S["sph_c"], S["sph_r"])
    if len(S["box_lo"]):
        b.set_boxes(S["box_lo"], S["box_hi"])


def assert_shape(S):
    """plant S, find the goal nodes by a first call without obstacles, bring the obstacles, re-check: everything the call leaves
    equals the reference, and so do the device's own check_motion verdicts"""
    ref = sh.reference(S)
    P, n = len(S["trees"]), sh.sizes(S)
    b = make_batch(S)
    plant(b, S)
    before = b.counts()
    r0 = b.revalidate_trees()
    assert not r0["n_removed"].any() and not r0["goal_lost"].any()
    assert list(b.counts()["goal_node"]) == [e["goal_before"] for e in ref]
    for p, (s, par) in enumerate(S["trees"]):
        gs, gp = b.tree(p)
        assert np.array_equal(bits(gs), bits(s)) and np.array_equal(gp, par), p
        new_index, edge_ok = b.revalidate_map(p)
        assert np.array_equal(new_index, np.arange(n[p])) and edge_ok.all(), p
    set_obstacles(b, S)
    for p, (s, par) in enumerate(S["trees"]):
        if n[p] > 1:
            frm, to = rh.edge_rows(s, par)
            got = np.asarray(b.check_motion(frm, to), dtype=bool)
            bad = np.flatnonzero(got != ref[p]["edge_ok"][1:]) + 1
            assert len(bad) == 0, "check_motion disagrees with the reference on problem %d, edges into %s" % (p, bad[:8])
    r = b.revalidate_trees()
    c = b.counts()
    print(S["name"], "n", n, "removed", list(r["n_removed"]), "goal", [e["goal_before"] for e in ref], "->", list(c["goal_node"]))
    for p, e in enumerate(ref):
        s, par = b.tree(p)
        assert s.shape[0] == e["n"] and np.array_equal(bits(s), bits(e["states"])), p
        assert np.array_equal(par, e["parents"]), p
        new_index, edge_ok = b.revalidate_map(p)
        assert len(new_index) == n[p] and np.array_equal(new_index, e["new_index"]), p
        assert np.array_equal(edge_ok.astype(bool), e["edge_ok"]), p
    assert list(r["n_removed"]) == [e["n_removed"] for e in ref] and list(c["nodes"]) == [e["n"] for e in ref]
    assert list(c["goal_node"]) == [e["goal_node"] for e in ref]
    assert [bool(v) for v in r["goal_lost"]] == [e["goal_lost"] for e in ref]
    assert (c["stop_reason"] == capi.STOP_NONE).all()
    for k in ("iterations", "accepted", "checksum"):
        assert np.array_equal(c[k], before[k]), k
    b.close()


# ------------------------------------------------------------------------------------------------ A .. F
@pytest.mark.parametrize("build", [sh.mixed_rn, sh.mixed_so3, sh.mixed_so2, sh.mixed_257], ids=lambda f: f.__name__)
def test_a_mixed_sizes_in_one_batch(build):
    assert_shape(build())


def test_b_survivors_move_by_whole_tiles():
    assert_shape(sh.moves())
    assert_shape(sh.move_256())


@pytest.mark.parametrize("leg", sh.c_legs(), ids=lambda leg: "r%d_%d_at%d%s" % (leg[0], leg[1], leg[2], "_boxes" if leg[3] else ""))
def test_c_sphere_windows(leg):
    assert_shape(sh.window_scene(*leg))


def test_d_steps_and_direction():
    assert_shape(sh.steps_scene())


@pytest.mark.parametrize("dim", sh.E_DIMS)
def test_e_outside_the_bounds(dim):
    assert_shape(sh.outside_scene(dim))


@pytest.mark.parametrize("which", ["a257", "b256"])
@pytest.mark.parametrize("k", range(len(sh.FRAMES)), ids=["x%g_plus%g" % f for f in sh.FRAMES])
def test_e_frames(which, k):
    assert_shape(sh.framed(which, k))


def test_f_the_goal_threshold_itself():
    assert_shape(sh.threshold_scene())


@pytest.mark.parametrize("space", ["rn", "so3", "so2"])
def test_f_the_goal_ladder(space):
    assert_shape(sh.ladder_scene(space))


# ------------------------------------------------------------------------------------------------ G, H: twins
def satisfied(space, states, goal):
    """goal.is_satisfied per state through entry points older than the call: distance(state, centre) <= radius"""
    if space == "so2":
        return np.array([h2.so2.distance(float(s[0]), float(goal[0][0])) <= goal[1] for s in states], dtype=bool)
    c = np.ascontiguousarray(np.broadcast_to(np.asarray(goal[0], dtype=np.float64), states.shape))
    d = capi.so3_op_batch(0, states, c) if space == "so3" else capi.distance_batch(states, c)
    return np.asarray(d).reshape(-1) <= goal[1]


def host_prune(b, space, goals):
    """the host loop the call replaces: get_tree, check_motion on every (parent, child) pair, prune in numpy, set_tree"""
    removed = []
    for p in range(b.n_problems):
        s, par = b.tree(p)
        edge_ok = np.ones(len(par), dtype=bool)
        if len(par) > 1:
            edge_ok[1:] = b.check_motion(*rh.edge_rows(s, par))
        exp = rh.expected(s, par, edge_ok, satisfied(space, s, goals[p]))
        b.set_tree(p, exp["states"], exp["parents"])
        removed.append(exp["n_removed"])
    return removed


def assert_same_trees(a, b):
    ca, cb = a.counts(), b.counts()
    for k in ("iterations", "accepted", "checksum", "nodes"):
        assert np.array_equal(ca[k], cb[k]), k
    for p in range(a.n_problems):
        (sa, pa), (sb, pb) = a.tree(p), b.tree(p)
        assert np.array_equal(bits(sa), bits(sb)) and np.array_equal(pa, pb), p


@pytest.mark.parametrize("kernel", [capi.KERNEL_RESIDENT, capi.KERNEL_LANES, capi.KERNEL_CELLS], ids=["resident", "lanes", "cells"])
def test_g_twins_lose_their_flag_when_the_lower_twin_dies(kernel):
    """goal_bias = 1: every sample is the goal centre, and the nearest node is the surviving upper twin -- unless it kept the skip
    flag that set_tree gave it, in which case it can never be nearest and the device-pruned batch grows another tree than the
    host-pruned one"""
    S = sh.twin_scene()
    ref = sh.reference(S)
    a, b = (make_batch(S, kernel, goal_bias=1.0, seed=5) for _ in range(2))
    for x in (a, b):
        plant(x, S)
        set_obstacles(x, S)
    removed = host_prune(b, "rn", S["goals"])
    r = a.revalidate_trees()
    assert list(r["n_removed"]) == removed == [e["n_removed"] for e in ref]
    assert_same_trees(a, b)
    for p, e in enumerate(ref):
        assert np.array_equal(bits(a.tree(p)[0]), bits(e["states"])), p
    a.solve(40)
    b.solve(40)
    assert_same_trees(a, b)
    for p, leg in enumerate(S["legs"]):
        _, groups, at_goal = sh.G_LEGS[leg]
        _, pa = a.tree(p)
        assert len(pa) > ref[p]["n"], leg
        assert pa[ref[p]["n"]] == ref[p]["new_index"][groups[at_goal][1]], leg   # the first new node hangs under the lowest surviving twin
    a.close()
    b.close()


def field_scene(dim=3, n_spheres=24, seed=0x5EED0100):
    start, goal = [0.5] * dim, [9.5] * dim
    r = 0.45 * math.sqrt(dim)
    return dict(dim=dim, bounds=[(0.0, 10.0)] * dim, max_distance=0.5, goal_bias=0.05, lvs_fraction=0.05, start=start, goal_centre=goal,
                goal_radius=0.5, boxes=None, spheres=scenarios.sphere_field(seed + dim, n_spheres, dim, 1.0, 9.0, 0.6 * r, r, [start, goal]))


H_P, H_MAX_NODES = 4, 1000
H_LEGS = {"stream": ("rn", capi.KERNEL_STREAM), "lanes": ("rn", capi.KERNEL_LANES), "cells": ("rn", capi.KERNEL_CELLS),
          "so3": ("so3", capi.KERNEL_AUTO), "so2": ("so2", capi.KERNEL_AUTO)}


def round_pair(leg):
    """-> (a, b, goals, set_field(batch, extra obstacle sites [k][dim]))"""
    space, kernel = H_LEGS[leg]
    if space == "rn":
        sc = field_scene()
        pair = [scenarios.make_batch(sc, H_P, H_MAX_NODES, False, 11, 0, 0, kernel) for _ in range(2)]
        goal = (np.array(sc["goal_centre"]), sc["goal_radius"])
        radii = [0.3, 0.35]

        def set_field(x, sites):
            x.set_spheres(np.concatenate([sc["spheres"][0], sites.reshape(-1, 3)]), np.concatenate([sc["spheres"][1], radii[:len(sites)]]))
    elif space == "so3":
        cone = (np.array([[0.0, 0.0, 0.0, 1.0]]), np.array([0.3]))
        start, target = rh.quat_axis_half([1.0, 0.0, 0.0], 0.6), rh.quat_axis_half([0.0, 1.0, 0.2], 0.7)
        pair = []
        for _ in range(2):
            x = capi.RRTBatch(4, sh.SO3_BOUNDS, 0.15, 0.05, H_P, H_MAX_NODES, 0.05, False, 11, space=capi.SPACE_SO3)
            x.set_spheres(*cone)
            x.setup(start, target, 0.1)
            pair.append(x)
        goal = (target, 0.1)

        def set_field(x, sites):
            x.set_spheres(np.concatenate([cone[0], sites.reshape(-1, 4)]), np.concatenate([cone[1], [0.05] * len(sites)]))
    else:
        sc = dict(h2.so2.fixture_scene(), max_nodes=H_MAX_NODES)
        pair = [h2.make_gpu(sc, H_P, 11, 0, stop_at_goal=False) for _ in range(2)]
        goal = (np.array([sc["target"]]), sc["goal_r"])

        def set_field(x, sites):
            mids = [h2.so2.normalise(float(v)) for v in sites.reshape(-1)]
            h2.set_arcs(x, list(sc["arcs"]) + [(max(m - 0.01, -h2.PI), min(m + 0.01, h2.PI)) for m in mids])
    return pair[0], pair[1], [goal] * H_P, set_field


@pytest.mark.parametrize("leg", sorted(H_LEGS))
def test_h_one_handle_round_after_round(leg):
    """three rounds of (two obstacles move onto the trees, re-check, solve), a round with the added obstacles gone, a round after
    problem 2 was cut down to ten nodes: the workspace of the earlier, larger calls is still there"""
    space = H_LEGS[leg][0]
    a, b, goals, set_field = round_pair(leg)
    a.solve(400)
    b.solve(400)
    assert_same_trees(a, b)

    def one_round(sites, label):
        for x in (a, b):
            set_field(x, sites)
        n_before = a.counts()["nodes"].copy()
        removed = host_prune(b, space, goals)
        r = a.revalidate_trees()
        print(leg, label, "nodes", list(n_before), "removed", list(r["n_removed"]))
        assert list(r["n_removed"]) == removed, label
        assert (a.counts()["stop_reason"] == capi.STOP_NONE).all()
        assert_same_trees(a, b)
        for p in range(H_P):
            new_index, edge_ok = a.revalidate_map(p)
            assert len(new_index) == len(edge_ok) == n_before[p] and int((new_index >= 0).sum()) == n_before[p] - removed[p], (label, p)
        a.solve(200)
        b.solve(200)
        assert_same_trees(a, b)
        return removed

    for k in range(3):
        trees = [a.tree(p)[0] for p in (k % H_P, (k + 1) % H_P)]
        sites = np.array([t[len(t) * (k + 1) // 4] for t in trees])
        assert sum(one_round(sites, "round %d" % k)) > 0
    assert sum(one_round(np.zeros((0, a.dim)), "obstacles gone")) == 0        # nothing removed, nothing comes back
    s, par = a.tree(2)
    for x in (a, b):
        x.set_tree(2, s[:10], par[:10])
    trees = [a.tree(p)[0] for p in (2, 0)]
    removed = one_round(np.array([trees[0][5], trees[1][len(trees[1]) // 2]]), "after shrinking problem 2")
    assert 0 < removed[2] < 10 and removed[0] > 0
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ the refused call
@pytest.mark.parametrize("planner", [capi.PLANNER_RRT_CONNECT, capi.PLANNER_RRT_STAR], ids=["connect", "star"])
def test_a_refused_call_leaves_extracted_paths_alone(planner):
    if planner == capi.PLANNER_RRT_CONNECT:
        x = scenarios.make_batch(scenarios.config2(), 4, 10000, True, 42, planner=planner)
        x.solve(200000)
    else:
        x = scenarios.make_batch(scenarios.config1(), 4, 4000, False, 42, planner=planner, search_radius=1.0)
        x.solve(3000)
    x.extract_paths()
    off, rows = x.paths()
    assert int(off[-1]) > 0
    with pytest.raises(capi.OxhipError) as e:
        x.revalidate_trees()
    assert e.value.status == capi.ERR_BAD_ARG and "revalidate_trees is for the RRT planner" in str(e.value)
    off2, rows2 = x.paths()
    assert np.array_equal(off, off2) and np.array_equal(bits(rows), bits(rows2))
    x.close()
