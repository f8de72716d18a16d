"""-m gpu: the batch-level services on SO(2) batches (OXHIP_SPACE_SO2): path extraction, the re-check after the arcs moved
(rrt_revalidate.hip over SeqSpace<-1>) and the shortcut (path_simplify.hip), each against plain host loops over the batch's own
get_tree / check_motion and the CPU checker (tests/golden/make_golden_so2.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import so2_helpers as h  # noqa: E402
from so2_helpers import so2  # noqa: E402
import rrt_revalidate_helpers as rv  # noqa: E402
from simplify_helpers import expected_checks, shortcut_dp  # noqa: E402
from oxmpl_amd import capi  # noqa: E402

P = 48


@pytest.fixture(scope="module")
def solved():
    sc = so2.fixture_scene()
    g = h.make_gpu(sc, P, 42, 0)
    assert (g.solve(2000) == capi.OK).all()
    return sc, g, [g.path(p).copy() for p in range(P)]


def test_get_paths_equals_get_path_of_every_problem(solved):
    sc, g, paths = solved
    g.extract_paths()
    off, rows = g.paths()
    assert int(off[P]) == sum(len(x) for x in paths) and rows.shape[1] == 1
    for p in range(P):
        assert np.array_equal(h.bits(rows[int(off[p]):int(off[p + 1])]), h.bits(paths[p])), p


def _pair_matrix(g, path):
    """valid(i, j) for every i < j by the batch's own check_motion, one call"""
    L = len(path)
    ij = [(i, j) for i in range(L) for j in range(i + 1, L)]
    ok = g.check_motion(np.array([path[i] for i, _ in ij]).reshape(-1, 1), np.array([path[j] for _, j in ij]).reshape(-1, 1)) if ij else []
    return {k: bool(v) for k, v in zip(ij, ok)}


def _assert_simplified(g, sc, paths, max_span):
    g.simplify_paths(max_span)
    off, rows, idx, raw, simp, checks = g.simplified_paths()
    arcs = so2.Arcs(sc["arcs"])
    shorter = 0
    for p, path in enumerate(paths):
        path = path.reshape(-1).tolist()
        L = len(path)
        valid = _pair_matrix(g, path)
        if p < 8:   # the batch's check_motion is the checker's (test_gpu_so2.py pins it on random rows; here on the path's own pairs)
            assert all(v == so2.check_motion(arcs, sc["fraction"], path[i], path[j]) for (i, j), v in valid.items())
            S = L - 1 if max_span == 0 else min(max_span, L - 1)
            m = g.path_valid_matrix(p, max_span)
            assert all(m[i, j] == v for (i, j), v in valid.items() if 2 <= j - i <= S)
        want_idx, want_raw, want_simp, _ = shortcut_dp(L, lambda i, j: valid[(i, j)], lambda i, j: so2.distance(path[i], path[j]), max_span)
        a, b = int(off[p]), int(off[p + 1])
        assert idx[a:b].tolist() == want_idx, p
        assert np.array_equal(h.bits(rows[a:b]).reshape(-1), h.bits(np.array([path[i] for i in want_idx])))
        assert h.bits(raw[p]) == h.bits(want_raw) and h.bits(simp[p]) == h.bits(want_simp), p
        assert int(checks[p]) == expected_checks(L, max_span)
        shorter += len(want_idx) < L
    return shorter


@pytest.mark.parametrize("max_span", [0, 3])
def test_simplify_equals_pair_matrix_plus_dp_on_wrapping_paths(solved, max_span):
    sc, g, paths = solved
    assert all(any(abs(a - b) > h.PI for a, b in zip(x.reshape(-1), x.reshape(-1)[1:])) for x in paths)   # every path wraps
    assert _assert_simplified(g, sc, paths, max_span) > P // 2   # and most of them get shorter


def test_simplify_paths_of_two_and_three_waypoints():
    """goal_bias 1: every sample is the target, so a start within max_distance gives the path (start, target) and one within twice
    that a path of three"""
    for start, want_len in ((1.45, 2), (1.25, 3)):
        sc = h.scene(max_distance=0.2, goal_bias=1.0, start=start, target=1.6, goal_r=0.01, arcs=[(-0.5, 0.5)])
        g = h.make_gpu(sc, 2, 1, 0)
        assert (g.solve(10) == capi.OK).all()
        paths = [g.path(p).copy() for p in range(2)]
        assert len(paths[0]) == want_len
        for span in (0, 1, 2):
            _assert_simplified(g, sc, paths, span)
        g.close()


def _host_revalidate(g, p, sc):
    """the host loop of tests/rrt_revalidate_helpers.py over get_tree / check_motion, against the arcs the batch holds now"""
    states, parents = g.tree(p)
    frm, to = rv.edge_rows(states, parents)
    edge_ok = np.concatenate([[True], g.check_motion(frm, to).astype(bool)]) if len(parents) > 1 else np.array([True])
    sat = [so2.distance(float(s), sc["target"]) <= sc["goal_r"] for s in states.reshape(-1)]
    return rv.expected(states, parents, edge_ok, sat)


def _assert_revalidated(g, p, want, out, goal_before):
    states, parents = g.tree(p)
    assert np.array_equal(h.bits(states), h.bits(want["states"])) and np.array_equal(parents, want["parents"]), p
    assert int(out["n_removed"][p]) == want["n_removed"] and int(g.counts()["goal_node"][p]) == want["goal_node"], p
    assert bool(out["goal_lost"][p]) == (goal_before >= 0 and want["goal_node"] < 0), p
    new_index, edge_ok = g.revalidate_map(p)
    assert np.array_equal(new_index, want["new_index"]) and np.array_equal(edge_ok, want["edge_ok"]), p


def test_revalidate_after_added_arcs_goal_lost_and_found_again():
    sc = so2.fixture_scene()
    n = 12
    g = h.make_gpu(sc, n, 42, 0)
    assert (g.solve(2000) == capi.OK).all()
    first = [so2.run_scene(sc, 42, p, max_iterations=2000) for p in range(n)]
    moved = dict(sc, arcs=sc["arcs"] + [(2.0, 2.2), (-2.6, -2.55)])   # across every solution path, and a sliver on the way
    h.set_arcs(g, moved["arcs"])
    want = [_host_revalidate(g, p, sc) for p in range(n)]
    out = g.revalidate_trees()
    for p in range(n):
        _assert_revalidated(g, p, want[p], out, first[p]["goal_node"])
    assert out["goal_lost"].all() and (out["n_removed"] > 0).all()
    # a second call finds nothing more to remove
    again = g.revalidate_trees()
    assert not again["n_removed"].any() and not again["goal_lost"].any()
    # the arcs move back: a further solve continues from the pruned trees, at the stream position the first solve left
    h.set_arcs(g, sc["arcs"])
    assert (g.solve(2000) == capi.OK).all()
    for p in range(n):
        cont = so2.run_scene(sc, 42, p, max_iterations=2000, tree=want[p]["states"].reshape(-1).tolist(), parents=want[p]["parents"].tolist(),
                             draws=first[p]["rng_draws"])
        states, parents = g.tree(p)
        assert np.array_equal(h.bits(states).reshape(-1), h.bits(np.array(cont["states"]))) and parents.tolist() == cont["parents"], p
        assert int(g.counts()["goal_node"][p]) == cont["goal_node"] >= 0
        assert np.array_equal(h.bits(g.path(p)).reshape(-1), h.bits(np.array(cont["path"])))
    g.close()


def test_revalidate_a_planted_tree_past_the_mirror():
    n = h.K_SO2_N + 1500
    rng = np.random.default_rng(4)
    parents = np.concatenate([[-1], [int(rng.integers(max(0, i - 40), i)) for i in range(1, n)]]).astype(np.int32)
    states = np.zeros(n)
    for i in range(1, n):   # short edges: a bushy tree around the start, -0.16 .. 0.36
        states[i] = states[parents[i]] + rng.uniform(-0.02, 0.02)
    target = float(states[n - 7])   # a goal region far up the tree
    sc = h.scene(max_distance=0.05, goal_bias=0.05, fraction=0.05, start=0.0, target=target, goal_r=1e-6, arcs=[], max_nodes=n + 100)
    g = h.make_gpu(sc, 2, 3, 0, stop_at_goal=False)
    g.set_tree(1, states.reshape(-1, 1), parents)
    out = g.revalidate_trees()   # no arcs: nothing goes, and the goal node is found
    assert not out["n_removed"].any() and int(g.counts()["goal_node"][1]) >= 1
    goal_before = int(g.counts()["goal_node"][1])
    arcs = [(0.3, 0.32), (-0.14, -0.13)]   # they cut 88 edges, and with them 247 nodes
    h.set_arcs(g, arcs)
    want = [_host_revalidate(g, p, sc) for p in range(2)]
    out = g.revalidate_trees()
    _assert_revalidated(g, 0, want[0], out, -1)
    _assert_revalidated(g, 1, want[1], out, goal_before)
    assert h.K_SO2_N < want[1]["n"] < n - 100   # a part went, and the tree still reaches past the mirror
    g.solve(64)   # and the planner goes on from the compacted tree (nothing was drawn before: the stream starts at its head)
    cont = so2.rrt_solve(sc["bounds"], sc["max_distance"], sc["goal_bias"], sc["fraction"], so2.Arcs(arcs), sc["start"], sc["target"],
                         sc["goal_r"], 3, 1, 64, sc["max_nodes"], stop_at_goal=False, tree=want[1]["states"].reshape(-1).tolist(),
                         parents=want[1]["parents"].tolist())
    got_states, got_parents = g.tree(1)
    assert cont["n"] > want[1]["n"] and got_parents.tolist() == cont["parents"]
    assert np.array_equal(h.bits(got_states).reshape(-1), h.bits(np.array(cont["states"])))
    g.close()
