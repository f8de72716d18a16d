"""CPU: the model of the dense shortcut (tests/prm_simplify_helpers.py) against section 18's model at m = 1, its invariants for
every m, and every limit shape held to its purpose -- with the CPU side's check_motion and distance as the checker."""
import random
import struct

import numpy as np
import pytest

import prm_simplify_helpers as ph
from simplify_helpers import shortcut_dp


def _bits(x):
    return struct.pack("<d", float(x))


def _lerp(a, b, t):
    return [x + (y - x) * t for x, y in zip(a, b)]


def _dist(a, b):
    return float(np.sqrt(sum((x - y) * (x - y) for x, y in zip(a, b))))


def _random_path(rng, L):
    return [[rng.uniform(0.0, 10.0), rng.uniform(0.0, 10.0)] for _ in range(L)]


@pytest.mark.parametrize("max_span", [0, 1, 2, 5])
def test_m1_is_the_waypoint_shortcut_on_random_matrices(max_span):
    rng = random.Random(7 + max_span)
    for L in (0, 1, 2, 3, 4, 9, 17):
        pts = _random_path(rng, L)
        table = {(i, j): rng.random() < 0.5 for i in range(L) for j in range(i + 2, L)}
        key = {tuple(p): i for i, p in enumerate(pts)}
        got = ph.dense_shortcut(pts, 1, max_span, lambda a, b: table[(key[tuple(a)], key[tuple(b)])], _dist, _lerp)
        idx, raw, simp, checks = shortcut_dp(L, lambda i, j: table[(i, j)], lambda i, j: _dist(pts[i], pts[j]), max_span)
        assert got["idx"] == idx and got["checks"] == checks
        assert _bits(got["raw"]) == _bits(raw) and _bits(got["simp"]) == _bits(simp)


@pytest.mark.parametrize("m", [1, 2, 3, 7, 16])
def test_invariants_for_every_m(m):
    rng = random.Random(100 + m)
    for L in (2, 3, 5, 8):
        for max_span in (0, 1, 2):
            pts = _random_path(rng, L)
            got = ph.dense_shortcut(pts, m, max_span, lambda a, b: rng.random() < 0.4, _dist, _lerp)
            M = (L - 1) * m + 1
            assert len(got["dense"]) == M and got["idx"][0] == 0 and got["idx"][-1] == M - 1     # both ends kept
            assert got["idx"] == sorted(set(got["idx"]))
            assert got["simp"] <= got["raw"]
            assert got["checks"] == ph.expected_checks(L, m, max_span)
            for k in range(L):                                                                     # q_{k m} is p_k itself
                assert [_bits(v) for v in got["dense"][k * m]] == [_bits(v) for v in pts[k]]
    assert ph.expected_checks(0, m, 0) == 0


def test_limit_shapes_are_held_to_their_purpose():
    shapes = ph.limit_shapes()
    models = {}
    for name, shape in shapes.items():
        pts, c, r, m, span, what = shape
        o = ph.oracle_checker(c, r)
        asked = []

        def valid(a, b, o=o, asked=asked):
            asked.append(bool(o.check_motion(a, b)))
            return asked[-1]

        from oracle import oracle_py as orc
        models[name] = got = ph.dense_shortcut(pts, m, span, valid, orc.distance, orc.interpolate)
        print("%-12s L=%d m=%d max_span=%d  M=%d  slots=%d  checks=%d (valid %d)  raw=%.6f simp=%.6f  idx=%s  -- %s"
              % (name, len(pts), m, span, len(got["dense"]), ph.matrix_bits(len(pts), m, span), got["checks"], sum(asked), got["raw"],
                 got["simp"], got["idx"], what))
        assert got["checks"] == len(asked) == ph.expected_checks(len(pts), m, span)
        assert all(o.is_valid(p) for p in pts)
        assert ph._dist2(pts[0], pts[1]) < ph.RADIUS ** 2 and (len(pts) < 3 or ph._dist2(pts[0], pts[2]) >= ph.RADIUS ** 2)
        if name.startswith("matrix_"):
            assert ph.matrix_bits(len(pts), m, span) == int(name.split("_")[1])
            assert any(asked) and not all(asked)          # a valid and an invalid checked pair
    assert models["corner_m8"]["simp"] < models["corner_m1"]["simp"] == models["corner_m1"]["raw"]
    assert models["short_L2_m1"]["checks"] == 0 and models["short_L2_m2"]["checks"] == 0 and models["short_L3_m1"]["checks"] == 1
    assert models["short_L2_m2"]["idx"] == [0, 2]
    # the tie: both chains exist, cost the same bits, and the model keeps the one through the lower index
    from oracle import oracle_py as orc
    pts = shapes["tie"][0]
    o = ph.oracle_checker(*shapes["tie"][1:3])
    assert not o.check_motion(pts[0], pts[3]) and o.check_motion(pts[0], pts[2]) and o.check_motion(pts[1], pts[3])
    via1 = orc.distance(pts[0], pts[1]) + orc.distance(pts[1], pts[3])
    via2 = orc.distance(pts[0], pts[2]) + orc.distance(pts[2], pts[3])
    assert _bits(via1) == _bits(via2) == _bits(models["tie"]["simp"])
    assert models["tie"]["idx"] == [0, 1, 3]
