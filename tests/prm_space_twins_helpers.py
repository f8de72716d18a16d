"""The scenes of tests/test_gpu_prm_space_twins.py and what the pure-Python restatement (tests/golden/make_golden.py,
make_golden_so3.py: distance, check_motion, Field / Cones) says about them: query sets, milestone validity, the re-checked edge
lists.  No GPU is needed here; tests/test_prm_space_twins_scenes.py checks on the CPU that no scene is vacuous.

A case is (space, n): space 1..8 is R^space, 0 is SO(3); n milestones drawn from a seeded generator, planted with a symmetric
ring and a few chords.  R^n: three spheres and one box, each about 5 % of the bounds' volume; SO(3): two cones."""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden as mg  # noqa: E402
import make_golden_so3 as so3  # noqa: E402

from prm_revalidate_helpers import plain_filter  # noqa: E402

SPACES = [1, 2, 3, 4, 5, 6, 7, 8, 0]
SIZES = [1, 256, 257]          # the i == 0 writer alone; the last lane of a block; the first lane of a second block
FRACTION = 0.05
SO3_UNBOUNDED = [0.0, 0.0, 0.0, 1.0, math.pi]
MAX_MILESTONES = 512


def ring_with_chords(n):
    """symmetric edge lists, ascending: i -- i + 1 all round, and a chord i -- i + 37 from every fifth milestone"""
    und = set()
    for i in range(n):
        for j in ([(i + 1) % n] + ([(i + 37) % n] if i % 5 == 0 else [])):
            if i != j:
                und.add((min(i, j), max(i, j)))
    lists = [[] for _ in range(n)]
    for a, b in und:
        lists[a].append(b)
        lists[b].append(a)
    return [sorted(r) for r in lists]


class Scene:
    pass


_SCENES = {}


def scene(space, n):
    if (space, n) in _SCENES:
        return _SCENES[(space, n)]
    rng = np.random.default_rng(20261019 + 100 * space + n)
    sc = Scene()
    sc.space, sc.n, sc.lists = space, n, ring_with_chords(n)
    if space == 0:
        unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)  # noqa: E731
        sc.dim, sc.bounds, sc.radius, sc.goal_radius = 4, SO3_UNBOUNDED, 1.0, 1.0
        sc.states = unit(rng.normal(size=(n, 4)))
        sc.sphere_c, sc.sphere_r = unit(rng.normal(size=(2, 4))), np.array([0.6, 0.5])
        sc.box_lo = sc.box_hi = np.zeros((0, 4))
        checker = so3.Cones(list(zip(sc.sphere_c.tolist(), sc.sphere_r.tolist())))
        sc.is_valid = checker.is_valid
        sc.distance = so3.distance
        sc.check_motion = lambda frm, to: so3.check_motion(checker, FRACTION, frm, to)
        draw = lambda: unit(rng.normal(size=4))  # noqa: E731
    else:
        d = space
        sc.dim, sc.bounds = d, [(0.0, 10.0)] * d
        sc.radius = sc.goal_radius = 3.5 * math.sqrt(d)
        sc.states = rng.uniform(0.5, 9.5, size=(n, d))
        ball = math.pi ** (d / 2.0) / math.gamma(d / 2.0 + 1.0)              # volume of the unit ball
        sc.sphere_c = rng.uniform(2.0, 8.0, size=(3, d))
        sc.sphere_r = np.full(3, 10.0 * (0.05 / ball) ** (1.0 / d))
        side = 10.0 * 0.05 ** (1.0 / d)
        sc.box_lo = rng.uniform(0.0, 10.0 - side, size=(1, d))
        sc.box_hi = sc.box_lo + side
        field = mg.Field(d, list(zip(sc.sphere_c.tolist(), sc.sphere_r.tolist())), list(zip(sc.box_lo.tolist(), sc.box_hi.tolist())))
        sc.is_valid = field.is_valid
        sc.distance = mg.distance
        sc.check_motion = lambda frm, to: mg.check_motion(field, sc.bounds, FRACTION, frm, to)
        draw = lambda: rng.uniform(0.5, 9.5, size=d)  # noqa: E731
    start = draw()
    while not sc.is_valid(start.tolist()):
        start = draw()
    # two queries: a valid start, and a start in the middle of the first obstacle
    sc.queries = [(start, draw()), (sc.sphere_c[0].copy(), draw())]
    _SCENES[(space, n)] = sc
    return sc


def expected_query(sc, start, goal):
    """(start valid, start connections, goal milestones) as prm.rs:243-264 finds them"""
    s, g = start.tolist(), goal.tolist()
    ms = sc.states.tolist()
    conn = [i for i, m in enumerate(ms) if sc.distance(s, m) < sc.radius and sc.check_motion(s, m)]
    goals = [i for i, m in enumerate(ms) if sc.distance(m, g) <= sc.goal_radius]
    return sc.is_valid(s), conn, goals


def expected_recheck(sc):
    """(valid mask, edge lists after the re-check, kept and removed undirected edges between valid milestones)"""
    ms = sc.states.tolist()
    valid = np.array([sc.is_valid(m) for m in ms], dtype=bool)
    ok = {(j, i): sc.check_motion(ms[j], ms[i]) for j, row in enumerate(sc.lists) for i in row if i < j and valid[i] and valid[j]}
    return valid, plain_filter(sc.lists, valid, ok), sum(ok.values()), len(ok) - sum(ok.values())


_EXPECTED = {}


def expected(space, n):
    """everything the restatement says about a case, computed once"""
    if (space, n) not in _EXPECTED:
        sc = scene(space, n)
        _EXPECTED[(space, n)] = dict(queries=[expected_query(sc, s, g) for s, g in sc.queries], recheck=expected_recheck(sc))
    return _EXPECTED[(space, n)]


def assert_not_vacuous(space, n):
    """from the restatement alone: both kinds of milestone in either query set, an invalid milestone, a removed and a kept edge"""
    e = expected(space, n)
    (sv0, conn, goals), (sv1, _, _) = e["queries"]
    valid, _, kept, removed = e["recheck"]
    assert sv0 and not sv1
    if n >= 256:
        assert 0 < len(conn) < n and 0 < len(goals) < n, (space, n, len(conn), len(goals))
        assert not valid.all() and valid.any(), (space, n)
        assert kept > 0 and removed > 0, (space, n, kept, removed)
