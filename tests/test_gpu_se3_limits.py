"""-m gpu: the SE(3) RRTConnect kernel (rrt_connect_se3.hip) at its limits, against the CPU checker (tests/golden/make_golden_se3.py)
bit for bit -- no tolerance anywhere.  The constructions are tests/se3_limits_shapes.py; that each has the property its test here
relies on is held on the CPU by tests/test_se3_limits_model.py.
  A  trees beyond the 256-node LDS mirror: the HBM tail of the nearest scan, nearest nodes read from HBM, launches that resume
     below, across and beyond the mirror's end; obstacles from LDS (81) and from HBM (169)
  B  motions with exactly ONE offending (state, body sphere, obstacle) triple, of 1 .. 129 states (up to three passes), 1 / 3 / 16 body
     spheres, 1 .. 200 obstacles: a triple the dealing over the lanes drops turns an invalid motion valid
  C  pairs at contact, an ulp either side, at the edges of the 2^-40 band; negative, zero-sum, infinite and NaN radii
  D  the wall scene scaled by 2^-30 and by 2^30
A, B and C also with the first kernel's sweep (DEBUG_SE3_BRANCHY_SWEEP), A with the stamped instantiation."""
import numpy as np
import pytest

import se3_limits_shapes as shapes
from oxmpl_amd import capi
from se3_helpers import assert_same, make_gpu

pytestmark = pytest.mark.gpu

se3 = shapes.se3
MODES = {"product": (0, False), "branchy": (capi.DEBUG_SE3_BRANCHY_SWEEP, False), "stamped": (0, True)}


def _gpu(sc, n_problems, seed, mode="product"):
    flags, stamped = MODES[mode]
    g = make_gpu(sc, n_problems, seed, 0, debug_flags=flags)
    if stamped:
        g.enable_stamps()
    return g


def _assert_full_trees_stay(g, results):
    """at the node cap: the stop reason, and a further solve call moves nothing and draws nothing"""
    st = g.solve(50)
    c = g.counts()
    for p, res in enumerate(results):
        assert int(c["stop_reason"][p]) == capi.STOP_NODES and int(st[p]) == capi.ERR_NO_SOLUTION_FOUND, p
        assert_same(g, p, res)


# ------------------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("variant", ["lds", "hbm"])
def test_wall_batch_beyond_the_mirror(variant, mode):
    results = [shapes.wall_run(variant, pid) for pid in shapes.WALL_PIDS]
    g = _gpu(shapes.wall_scene(variant), len(results), shapes.WALL_SEED, mode)
    st = g.solve(shapes.BUDGET)
    c = g.counts()
    for p, res in enumerate(results):
        assert min(res["n"]) > shapes.MIRROR
        assert_same(g, p, res)
        assert int(c["stop_reason"][p]) == capi.STOP_NODES and int(st[p]) == capi.ERR_NO_SOLUTION_FOUND, p
    _assert_full_trees_stay(g, results)
    g.close()


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("variant", ["lds", "hbm"])
def test_wall_resumed_across_the_mirror(variant, mode):
    """problem 0 in launches of 97 iterations (and one stop where the trees straddle the mirror's end): every launch reloads the first
    256 nodes only, the later ones start with trees that reach beyond them"""
    res = shapes.wall_run(variant, 0)
    below, straddle = shapes.WALL_BELOW[variant], shapes.WALL_STRADDLE[variant]
    stops = sorted(set(range(shapes.CUT, res["iterations"] + 2 * shapes.CUT, shapes.CUT)) | {straddle})
    g = _gpu(shapes.wall_scene(variant), 1, shapes.WALL_SEED, mode)
    done = 0
    for stop in stops:
        g.solve(stop - done)
        done = stop
        if stop in (below, straddle):
            assert_same(g, 0, shapes.wall_run(variant, 0, stop))
    assert_same(g, 0, res)
    _assert_full_trees_stay(g, [res])
    g.close()


# ------------------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("mode", ["product", "branchy"])
@pytest.mark.parametrize("n_obs", shapes.B_NOBS)
@pytest.mark.parametrize("nbody", shapes.B_NBODY)
def test_one_offending_triple_in_the_planner(nbody, n_obs, mode):
    sc, problems = shapes.b_batch(nbody, n_obs)
    expected = shapes.b_expected(nbody, n_obs)
    g = _gpu(sc, len(problems), 0, mode)
    g.solve(2)
    c, gc = g.counts(), g.goal_counts()
    for p, (prob, (res, _)) in enumerate(zip(problems, expected)):
        assert_same(g, p, res, c, gc)
        if prob["control"]:       # the motion start -> target is valid: inserted, and the goal reached with it
            assert int(c["goal_node"][p]) == 1 and int(c["iterations"][p]) == 1 and int(c["stop_reason"][p]) == capi.STOP_GOAL, prob
        else:                     # the one triple refuses it, twice
            assert [int(c["nodes"][p]), int(gc["nodes"][p])] == [1, 1] and int(c["iterations"][p]) == 2 and int(c["goal_node"][p]) < 0, prob
    g.close()


@pytest.mark.parametrize("mode", ["product", "branchy"])
@pytest.mark.parametrize("n_obs", shapes.B_NOBS)
@pytest.mark.parametrize("nbody", shapes.B_NBODY)
def test_one_offending_triple_in_check_motion(nbody, n_obs, mode):
    """the stand-alone hook reads the obstacles from HBM whatever their number"""
    sc, problems = shapes.b_batch(nbody, n_obs)
    want = [motion for _, motion in shapes.b_expected(nbody, n_obs)]
    assert want == [prob["control"] for prob in problems]
    g = _gpu(shapes.problem_scene(sc, 0), 1, 0, mode)
    got = g.check_motion(np.array(sc["start"]), np.array(sc["target"])).tolist()
    assert got == want, [prob for prob, a, b in zip(problems, got, want) if a != b]
    g.close()


# ------------------------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("mode", ["product", "branchy"])
@pytest.mark.parametrize("place", shapes.C_PLACES)
def test_contact_and_unusual_radii(place, mode):
    seen = set()
    for name, sc in list(shapes.c_contact_cases(place)) + list(shapes.c_radius_cases(place)):
        want = shapes.c_expected(sc)
        g = _gpu(sc, 2, 0, mode)
        state = sc["target"][0]
        assert g.is_valid(np.array([state])).tolist() == [want["valid"]], name
        assert g.check_motion(np.array(sc["start"]), np.array(sc["target"])).tolist() == want["motions"] == [want["valid"]] * 2, name
        g.solve(2)
        for p in range(2):
            assert (want["runs"][p]["end"][0] >= 0) == want["valid"], name
            assert_same(g, p, want["runs"][p])
        g.close()
        seen.add(want["valid"])
    assert seen == {True, False}


# ------------------------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize("frame", sorted(shapes.FRAMES))
def test_scaled_frames(frame):
    results = [shapes.frame_run(frame, pid) for pid in shapes.FRAME_PIDS]
    g = _gpu(shapes.frame_scene(frame), len(results), shapes.WALL_SEED)
    g.solve(shapes.BUDGET)
    c = g.counts()
    for p, res in enumerate(results):
        assert min(res["n"]) > 60
        assert_same(g, p, res)
        assert int(c["stop_reason"][p]) == capi.STOP_NODES, p
    g.close()
