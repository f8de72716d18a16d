"""-m gpu: rrt_so2.hip at the smallest shapes at which it can go wrong (tests/so2_limits_shapes.py; tests/test_so2_limits_model.py
holds every shape to its purpose on the CPU): trees around the LDS mirror's size, exact ties and the +-PI seam in the nearest
search, arc counts around the staged table's size, motions around the 64-state pass, rejected range draws, launch cuts inside a
sampled block and the stops.  Every planner shape is compared with the checker bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import so2_helpers as h  # noqa: E402
import so2_limits_shapes as shapes  # noqa: E402
from so2_helpers import so2  # noqa: E402
from oxmpl_amd import capi  # noqa: E402

PLANNER = shapes.planner_shapes()


def _run_on_gpu(shape, n_problems=1):
    sc = shape["sc"]
    g = h.make_gpu(sc, n_problems, shape["seed"], shape["pid"], stop_at_goal=shape.get("stop_at_goal", True))
    if shape.get("tree") is not None:
        g.set_tree(0, np.array(shape["tree"]).reshape(-1, 1), shape["parents"])
    for step in shape.get("cuts", [shape["iterations"]]):
        g.solve(step)
    return g


@pytest.mark.parametrize("name", sorted(PLANNER))
def test_planner_shape_equals_the_checker(name):
    shape = PLANNER[name]
    assert sum(shape.get("cuts", [shape["iterations"]])) == shape["iterations"]
    g = _run_on_gpu(shape)
    h.assert_same(g, 0, shapes.run(shape))
    g.close()


def test_a_nan_node_cannot_be_planted():
    """rrt_so2.hip keeps node 0 when its distance is NaN, as rrt_so3.hip does, but no entry point lets a NaN into a tree: setup and
    set_tree refuse non-finite states (at index 0 and at index 5 alike), and the arithmetic makes none from finite ones"""
    sc = h.scene()
    g = h.make_gpu(sc, 1, 0, 0)
    for idx in (0, 5):
        states = np.linspace(0.0, 1.0, 8)
        states[idx] = np.nan
        with pytest.raises(capi.OxhipError) as ei:
            g.set_tree(0, states.reshape(-1, 1), [-1] + [0] * 7)
        assert ei.value.status == capi.ERR_BAD_ARG
    with pytest.raises(capi.OxhipError) as ei:
        g.setup([np.nan], [1.0], 0.1)
    assert ei.value.status == capi.ERR_BAD_ARG
    g.close()


def test_validity_rows_closed_ends_and_the_arc_over_the_seam():
    arcs, rows = shapes.validity_rows()
    g = h.make_gpu(h.scene(arcs=arcs), 1, 0, 0)
    got = g.is_valid(np.array([v for v, _ in rows]).reshape(-1, 1)).astype(bool)
    assert got.tolist() == [want for _, want in rows]
    # a motion across the seam through the arc that contains -PI, and one that stays clear of it
    assert g.check_motion(np.array([[3.0], [2.0]]), np.array([[-2.9], [2.9]])).astype(bool).tolist() == [False, True]
    g.close()


def test_arc_counts_around_the_staged_table():
    """is_valid / check_motion with 0, 1, KA and KA + 1 arcs, the deciding arc last"""
    for count in (0, 1, shapes.KA, shapes.KA + 1):
        arcs = shapes._slivers(count - 1) + [(0.55, 0.65)] if count else []
        g = h.make_gpu(h.scene(arcs=arcs), 1, 0, 0)
        want = count == 0
        # (states inside the arc: its closed ends are test_validity_rows' business -- 0.55 normalises a hair below 0.55)
        assert g.is_valid(np.array([[0.6], [0.5], [0.56], [0.64]])).astype(bool).tolist() == [want, True, want, want]
        assert g.check_motion(np.array([[0.5], [0.4]]), np.array([[0.7], [0.5]])).astype(bool).tolist() == [want, True]
        g.close()


def test_motion_rows_around_the_64_state_pass():
    for arcs, frm, to, n, first_bad in shapes.motion_rows():
        g = h.make_gpu(h.scene(arcs=arcs, fraction=0.05), 1, 0, 0)
        assert bool(g.check_motion(np.array([[frm]]), np.array([[to]]))[0]) == (first_bad is None), (n, first_bad)
        g.close()


def test_max_nodes_mid_block_leaves_the_stream_where_the_loop_does():
    """the tree fills at iteration 39 of a sampled block of 64; the stream position the stop leaves is not readable, so a frozen
    launch (which ignores the node cap) continues from it: its checksum folds in the samples drawn from that position on"""
    shape = PLANNER["max_nodes_mid_block"]
    sc = shape["sc"]
    first = shapes.run(shape)
    g = _run_on_gpu(shape)
    h.assert_same(g, 0, first)
    assert int(g.counts()["stop_reason"][0]) == 2 and int(g.counts()["iterations"][0]) % 64 != 0
    g.solve(50)   # full: nothing runs
    h.assert_same(g, 0, first)
    g.solve(30, freeze=True)
    frozen = so2.rrt_solve(sc["bounds"], sc["max_distance"], sc["goal_bias"], sc["fraction"], so2.Arcs(sc["arcs"]), sc["start"], sc["target"],
                           sc["goal_r"], shape["seed"], shape["pid"], 30, sc["max_nodes"], freeze=True, tree=first["states"],
                           parents=first["parents"], draws=first["rng_draws"])
    Pm = pow(so2.mg.FNV_P, 30, 1 << 64)
    want = (first["checksum"] * Pm + frozen["checksum"] - so2.mg.FNV_BASIS * Pm) & so2.M64
    c = g.counts()
    assert int(c["iterations"][0]) == first["iterations"] + 30 and int(c["checksum"][0]) == want and int(c["nodes"][0]) == first["n"]
    g.close()


def test_solve_again_after_a_solved_problem_changes_nothing():
    sc = so2.fixture_scene()
    want = so2.run_scene(sc, 42, 5, max_iterations=2000)
    g = h.make_gpu(sc, 1, 42, 5)
    assert g.solve(2000)[0] == capi.OK
    h.assert_same(g, 0, want)
    assert g.solve(500)[0] == capi.OK and g.solve(1)[0] == capi.OK
    h.assert_same(g, 0, want)
    g.close()
