"""CPU: the constructions of tests/se3_limits_shapes.py hold what tests/test_gpu_se3_limits.py needs them to hold, by the checker
(tests/golden/make_golden_se3.py) alone.  The GPU test compares every one of these runs with the checker bit for bit, so the
conditions carry over to the device's run: the wall problems end at the node cap with both trees beyond the 256-node mirror and
nearest nodes found there; the resumed run is compared below the mirror and across its end; every offender motion has exactly one
offending (state, body sphere, obstacle) triple, its control none, each with the intended number of states; the contact sweeps give
both verdicts; the scaled frames grow real trees."""
import math

import numpy as np
import pytest

import se3_limits_shapes as shapes
from helpers import bits

se3 = shapes.se3


# ------------------------------------------------------------------------------------------------------------ A and D
@pytest.mark.parametrize("variant", ["lds", "hbm"])
def test_wall_problems_end_at_the_cap_beyond_the_mirror(variant):
    sc = shapes.wall_scene(variant)
    assert (len(sc["obstacles"]) > shapes.LDS_OBS) == (variant == "hbm")
    first_beyond = 0
    for pid in shapes.WALL_PIDS:
        res = shapes.wall_run(variant, pid)
        print(variant, pid, res["n"], res["iterations"], "parents beyond the mirror", shapes.far_parents(res))
        assert res["end"] == [-1, -1] and max(res["n"]) == sc["max_nodes"] and res["iterations"] < shapes.BUDGET   # the cap, unsolved
        assert min(res["n"]) > shapes.MIRROR
        assert shapes.far_parents(res) >= 10
        first_beyond += sum(1 for t in res["parents"] for v in t if v == shapes.MIRROR)
    assert first_beyond >= 1                                   # node 256 itself, the first that is in HBM only, is a nearest node


@pytest.mark.parametrize("variant", ["lds", "hbm"])
def test_wall_checkpoints_of_the_resumed_run(variant):
    below, straddle, end = shapes.WALL_BELOW[variant], shapes.WALL_STRADDLE[variant], shapes.wall_run(variant, 0)["iterations"]
    assert below % shapes.CUT == 0 and below < straddle < end
    n = shapes.wall_run(variant, 0, below)["n"]
    assert max(n) < shapes.MIRROR and min(n) > shapes.MIRROR - 64          # below, and not far below
    n = shapes.wall_run(variant, 0, straddle)["n"]
    assert min(n) <= shapes.MIRROR <= max(n) and n[0] != n[1]
    # the launches of CUT iterations start below, across and beyond the mirror's end
    assert (straddle // shapes.CUT + 1) * shapes.CUT < end


@pytest.mark.parametrize("frame", sorted(shapes.FRAMES))
def test_scaled_frames_grow_trees(frame):
    sc = shapes.frame_scene(frame)
    k = shapes.FRAMES[frame]
    assert sc["bounds_xyz"][0] == (-3.0 * k, 3.0 * k) and sc["max_distance"] == 0.5 * k and sc["obstacles"][0][1] == 0.8 * k
    for pid in shapes.FRAME_PIDS:
        res = shapes.frame_run(frame, pid)
        print(frame, pid, res["n"], res["iterations"])
        assert min(res["n"]) > 60 and res["end"] == [-1, -1]
    # which term of the distance decides: at 2^-30 a step of max_distance is all rotation, at 2^30 all translation
    a, b = sc["start"], sc["target"]
    d_xyz, d_q = se3.mg.distance(a[:3], b[:3]), shapes.so3.distance(a[3:], b[3:])
    assert (d_xyz < 1e-6 * d_q) if frame == "down" else (d_q < 1e-6 * d_xyz)


# ------------------------------------------------------------------------------------------------------------ B
def test_one_triple_grid_is_whole():
    assert sorted(shapes.B_STEPS) == [1, 2, 4, 5, 64, 65, 129]
    for S, picks in shapes.B_STEPS.items():
        assert set(picks) == {s for s in (1, 64, 65, S) if s <= S} | ({128} if S == 129 else set())
        frm, to = shapes.b_motion(S)
        assert se3.distance(frm, to) <= 3.0
    kinds = set()
    for nbody in shapes.B_NBODY:
        for n_obs in shapes.B_NOBS:
            sc, problems = shapes.b_batch(nbody, n_obs)
            assert 2 * sum(len(v) for v in shapes.B_STEPS.values()) <= len(problems) <= 400
            assert {p["b"] for p in problems} == {0, nbody - 1}
            assert {p["j"] for p in problems} == {j for j in (0, 37, n_obs - 1) if j < n_obs}
            for p in problems:   # lanes per pair in the pass that holds s*, and its rounds
                ch = min(64, p["S"] - (p["s"] - 1) // 64 * 64)
                g = 64
                while g > 1 and ch * nbody * g > 64:
                    g //= 2
                kinds.add((g, ch * nbody > 64, n_obs < g, ch * nbody * g < 64))
    assert {k[0] for k in kinds} == {64, 32, 16, 8, 4, 2, 1}
    assert any(k[1] for k in kinds) and any(k[2] for k in kinds) and any(k[3] for k in kinds)   # rounds; lanes with no obstacle; idle lanes


@pytest.mark.parametrize("n_obs", shapes.B_NOBS)
@pytest.mark.parametrize("nbody", shapes.B_NBODY)
def test_one_offending_triple_each(nbody, n_obs):
    sc, problems = shapes.b_batch(nbody, n_obs)
    near = [c for c, r in sc["obstacles"] if r == 1e-4]
    assert all(se3.mg.distance(a, b) >= 10.0 for i, a in enumerate(near) for b in near[:i])
    assert all(c[0] >= 1000.0 for c, r in sc["obstacles"] if r != 1e-4)
    for p, prob in enumerate(problems):
        frm, to = sc["start"][p], sc["target"][p]
        assert se3.distance(frm, to) <= sc["max_distance"]
        assert shapes.steps(sc, frm, to) == prob["S"], prob
        want = [] if prob["control"] else [(prob["s"], prob["b"], prob["j"])]
        assert shapes.offending_triples(sc, frm, to) == want, prob


# ------------------------------------------------------------------------------------------------------------ C
def _cases(place):
    return list(shapes.c_contact_cases(place)) + list(shapes.c_radius_cases(place))


@pytest.mark.parametrize("place", shapes.C_PLACES)
def test_contact_cases(place):
    n_obs, index = place
    verdicts = {}
    for name, sc in _cases(place):
        body = se3.make_body(sc)
        state = sc["target"][0]
        assert len(sc["obstacles"]) == n_obs and sum(1 for c, _ in sc["obstacles"] if c[0] < 1000.0) == 1
        for p, want in enumerate((1, 70)):
            states = shapes.motion_states(sc, sc["start"][p], state)
            assert len(states) == want and se3.distance(sc["start"][p], state) <= sc["max_distance"]
            assert np.array_equal(bits(states[-1]), bits(state)), name           # the state is the motion's last, bit for bit
            for s in states:
                assert body.is_valid(s) == body.is_valid_scalar(s), name
            if all(math.isfinite(r) for _, r in sc["obstacles"]):
                assert all(body.is_valid(s) for s in states[:-1]), name           # ... and alone decides the motion
        verdicts[name] = body.is_valid(state)
    for pose, (state, near, at) in shapes.C_POSES.items():
        assert np.array_equal(bits(se3.body_centre(state, shapes.C_BODY[near][0])), bits(at))   # exactly there
        sweep = [verdicts["%s eps %+.3g" % (pose, eps)] for eps in shapes.C_EPS]
        assert set(sweep) == {True, False}, pose
        assert sweep[0] is False and sweep[-1] is True                           # contact is a hit (strict >), 2^-30 away is none
    # at x = 0 an ulp either side of contact is told apart
    assert verdicts["zero eps %+.3g" % 2.0 ** -52] is True and verdicts["zero eps %+.3g" % -2.0 ** -52] is False
    want = {"sum 0, d2 0": False, "sum 0, d2 > 0": True, "sum < 0, d2 0": True, "sum < 0, d2 > 0": True, "-inf, d2 0": True, "-inf": True,
            "+inf": False, "+inf far": False, "nan": False, "nan, d2 0": False, "nan far": False, "point on point": False,
            "point near point": True, "point at contact": False, "point inside the band": True, "point outside the band": True,
            "point an ulp inside": False}
    assert {k: verdicts[k] for k in want} == want
