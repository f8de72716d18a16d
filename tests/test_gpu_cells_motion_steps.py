"""-m gpu: the back half of a cell-grid round (rrt_cells.hip) -- midpoint filter and motion check -- against the
oracle bit for bit: node counts, iteration counts, accepted counts, checksums, trees.

The lanes' own motion check takes the step fractions s / n of motions of up to 8 steps from a table in LDS and walks a lane's
spheres in the outer loop, the steps inside (motion_own_lane_short, lane_query_common.hpp); a wave with a longer motion takes
the loop that divides in every step.  The scenes vary what those loops branch on:

* the step count of a full motion, through lvs_fraction at max_distance 0.5 (res = fraction x extent x 0.1; the fraction is
  chosen so that max_distance / res = n - 1/2): 1 and 2, the benchmark's own 0.05 (6 steps in R^3, 8 in R^2), 8 -- the table's
  last row --, 9 -- the first wave that falls back -- and 20;
* unequal step counts inside one wave: goal_bias 0.5 with the goal centre 0.2 from a node, so half of the motions are short;
* the spheres: none, one, 64, 80 (16 go through the loop over the obstacles beyond the first 64), two and a box, a stack
  of overlapping spheres that gives a lane many bits to walk, and a tree with nodes outside the bounds, where the midpoint
  lies outside the filter's grid and every sphere is a candidate.

Every case: P = 4 trees handed in through set_tree (about 1,400 nodes in R^3, 1,000 in R^2: a grid is in use), 448 frozen
iterations with frozen_split 1 and 3, then one growing leg, which the shared function serves too.  In every scene with
obstacles the oracle alone must accept and reject at least 10 % of the frozen leg's motions: a check that only ever accepts
would prove nothing."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oxmpl_amd import capi  # noqa: E402
from oracle import oracle_py as orc  # noqa: E402
import test_gpu_cells_limits as model  # noqa: E402

P = 4
MAX_NODES = 4000
N_TREE = {2: 1000, 3: 1400}
LEGS = ((448, True), (160, False))
SPLITS = (1, 3)
MAX_DISTANCE = 0.5
BENCH = 0            # "the benchmark's own lvs_fraction"


def _fraction(dim, steps, lo=0.0, hi=10.0):
    """lvs_fraction for which a motion of length max_distance takes `steps` steps: max_distance / res = steps - 1/2"""
    if steps == BENCH:
        return 0.05
    extent = float(np.sqrt(dim * (hi - lo) ** 2))
    return MAX_DISTANCE / ((steps - 0.5) * 0.1 * extent)


def _full_steps(dim, fraction, lo=0.0, hi=10.0):
    return int(np.ceil(MAX_DISTANCE / (fraction * float(np.sqrt(dim * (hi - lo) ** 2)) * 0.1)))


def _spheres(rng, dim, n, rmin, rmax, lo=0.0, hi=10.0):
    return lo + rng.random((n, dim)) * (hi - lo), rmin + rng.random(n) * (rmax - rmin)


def _obstacles(kind, dim):
    """(spheres, boxes) of the scene `kind`"""
    rng = np.random.default_rng(4100 + dim)
    if kind == "none":
        return None, None
    if kind == "one":
        return (np.array([[5.0] * dim]), np.array([3.6 if dim == 3 else 2.6])), None
    if kind == "s64":
        return _spheres(rng, dim, 64, 0.6, 1.3 if dim == 3 else 0.8), None
    if kind == "s80":
        return _spheres(rng, dim, 80, 0.6, 1.2 if dim == 3 else 0.7), None
    if kind == "box":
        return (np.array([[2.0] * dim, [8.0] + [2.0] * (dim - 1)]), np.array([1.5, 1.2])), (np.array([[2.5] * dim]), np.array([[8.5] * dim]))
    if kind == "stack":
        # five piles of eight spheres each, centres within 0.15 of the pile's, radii 1.0 .. 1.9: whatever motion comes near a
        # pile passes the midpoint filter of several of its spheres at once
        piles = 2.0 + rng.random((5, dim)) * 6.0
        c = np.repeat(piles, 8, axis=0) + (rng.random((40, dim)) - 0.5) * 0.3
        return (c, 1.0 + rng.random(40) * (0.9 if dim == 3 else 0.4)), None
    if kind == "outside":
        return _spheres(rng, dim, 64, 0.8, 1.6 if dim == 3 else 1.0, -3.0, 13.0), None
    raise ValueError(kind)


def _scene(kind, dim, steps, goal_near=False):
    spheres, boxes = _obstacles(kind, dim)
    if goal_near:
        # the first sphere moves next to the short motion (1, 1, ..) -> (1.2, 1, ..): 0.6 away from it, radius 0.5 -- the
        # midpoint filter keeps it, no step touches it, so the short lanes walk their steps beside the full ones
        # (and the spheres that would cover it are mirrored to the far corner)
        c, r = spheres[0].copy(), spheres[1].copy()
        cover = np.sqrt(((c - np.array([1.1] + [1.0] * (dim - 1))) ** 2).sum(axis=1)) < r + 0.45
        c[cover] = 10.0 - c[cover]
        c[0], r[0] = [1.1, 1.6] + [1.0] * (dim - 2), 0.5
        spheres = (c, r)
    return dict(dim=dim, bounds=[(0.0, 10.0)] * dim, max_distance=MAX_DISTANCE, goal_bias=0.5 if goal_near else 0.05,
                lvs_fraction=_fraction(dim, steps), start=[1.0] * dim,
                goal_centre=[1.2] + [1.0] * (dim - 1) if goal_near else [9.0] * dim, goal_radius=0.3, spheres=spheres, boxes=boxes)


def _trees(kind, dim):
    rng = np.random.default_rng(4200 + dim)
    lo, hi = (-3.0, 13.0) if kind == "outside" else (0.0, 10.0)
    out = []
    for _ in range(P):
        s, par = model._random_tree(rng, N_TREE[dim], lo, hi, dim)
        s[0] = 1.0                               # (the start)
        out.append((s, par))
    assert model.cells_level(N_TREE[dim], dim, model.cells_level_max(dim, MAX_NODES)) > 0     # a grid, not the brute list
    return out


def _want(key, sc, trees):
    def make():
        planners = [model._oracle(sc, 11, 300 + p, MAX_NODES, False) for p in range(P)]
        for o, (s, par) in zip(planners, trees):
            assert o.set_tree(s, par) == 0
        return planners
    return model._oracle_legs(("motion_steps",) + key, make, LEGS, 4)


def _check(kind, dim, steps, goal_near=False):
    sc = _scene(kind, dim, steps, goal_near)
    trees = _trees(kind, dim)
    want = _want((kind, dim, steps, goal_near), sc, trees)
    if kind != "none":
        # non-vacuity, from the oracle alone: the frozen leg both accepts and rejects
        it = sum(w["iterations"] for w in want[0])
        acc = sum(w["accepted"] for w in want[0])
        print("%s R^%d steps %d goal_near %d: oracle accepted %d of %d frozen iterations" % (kind, dim, steps, goal_near, acc, it))
        assert it == P * LEGS[0][0]
        assert 0.1 * it <= acc <= 0.9 * it, (acc, it)
    else:
        assert all(w["accepted"] == w["iterations"] for w in want[0])
    assert all(w["nodes"] > N_TREE[dim] for w in want[1])            # the growing leg grew every tree
    for split in SPLITS:
        gpu = model._gpu(sc, P, MAX_NODES, False, 11, 300, frozen_split=split)
        for p, (s, par) in enumerate(trees):
            gpu.set_tree(p, s, par)
        model._run_legs(gpu, LEGS, want, P)
        gpu.close()


def test_step_fractions_span_the_table():
    """the fractions chosen give the step counts named: 1, 2, 8 (the table's last row), 9 (the first fallback), 20, and the
    benchmark's 6 (R^3) and 8 (R^2)"""
    for dim in (2, 3):
        for steps in (1, 2, 8, 9, 20):
            f = _fraction(dim, steps)
            assert 0.0 < f <= 1.0 and _full_steps(dim, f) == steps
    assert _full_steps(3, 0.05) == 6 and _full_steps(2, 0.05) == 8


@pytest.mark.parametrize("steps", [1, 2, BENCH, 8, 9, 20], ids=lambda s: "bench" if s == BENCH else "steps%d" % s)
@pytest.mark.parametrize("kind", ["s64", "s80"])
@pytest.mark.parametrize("dim", [2, 3])
def test_step_counts(dim, kind, steps):
    """64 spheres (all in LDS) and 80 (16 beyond them, walked step by step): every step count on either side of the table's end"""
    _check(kind, dim, steps)


@pytest.mark.parametrize("steps", [BENCH, 9], ids=["bench", "steps9"])
@pytest.mark.parametrize("kind", ["s64", "s80"])
@pytest.mark.parametrize("dim", [2, 3])
def test_unequal_step_counts_in_one_wave(dim, kind, steps):
    """half of a wave's motions end at the goal centre, 0.2 from the start node: 3 steps (bench) or 4 (steps9) beside the full
    motions' 6 / 8 / 9 -- in the last case the short lanes go through the fallback with the long ones"""
    _check(kind, dim, steps, goal_near=True)


@pytest.mark.parametrize("kind", ["none", "one", "box", "stack", "outside"])
@pytest.mark.parametrize("dim", [2, 3])
def test_sphere_counts(dim, kind):
    """no obstacle, one sphere, spheres and a box, piles of overlapping spheres, a tree that reaches outside the bounds"""
    _check(kind, dim, BENCH)


@pytest.mark.parametrize("dim", [2, 3])
def test_overlapping_spheres_give_a_lane_three_bits(dim):
    """the `stack` scene does what it is for (host arithmetic only): of the oracle-style motions from the trees' nodes, a good
    part has three or more spheres within reach of its midpoint (|mid - c| <= r + half the motion's length)"""
    (c, r), _ = _obstacles("stack", dim)
    rng = np.random.default_rng(7)
    s, _ = _trees("stack", dim)[0]
    d = rng.normal(size=s.shape)
    mid = s + 0.25 * d / np.sqrt((d * d).sum(axis=1))[:, None]
    reach = (np.sqrt(((mid[:, None, :] - c[None, :, :]) ** 2).sum(axis=2)) <= r[None, :] + 0.25).sum(axis=1)
    assert (reach >= 3).mean() > 0.1, (reach >= 3).mean()
