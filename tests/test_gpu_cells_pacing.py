"""-m gpu: the pacing of a frozen cell-grid launch (rrt_cells.hip) changes who issues when and nothing else.

Every wave of a frozen launch reports its progress to a board (one counter per XCD) and takes its issue priority from where it
stands against the XCD's mean.  So every case here is compared bit for bit -- iterations, nodes, accepted, checksum -- with the
CPU oracle (freeze = True), and run a second time under OXHIP_DEBUG_CELLS_NO_PACING (the reports still run, no wave changes
its priority), which must give the same.  What varies is what the board's arithmetic and its reset depend on:

* R^2 and R^3; trees of 300 nodes (the flat list) and 700 (a grid), handed in through set_tree;
* P in {1, 3, 9, 17}: dead waves in the only workgroup, a last workgroup that is not full, XCDs without a problem;
  frozen_split in {1, 2, 3, 4, 8} (up to 4 parts skip to their own starts, 8 go through the prepare pass);
* budgets 1, 63, 64, 65, 200, 1000, one frozen launch after the other on one batch: fewer rounds than parts, a last round that
  is not full, and both boards in turn, each cleared by the launch before;
* two batches stepped alternately, a growing launch between two frozen ones, a launch whose problems have reached their goal;
* the stamped build: when a launch is over, its board holds, summed over the XCDs, the quota of every live problem."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oxmpl_amd import capi  # noqa: E402
from oracle import oracle_py as orc  # noqa: E402
import test_gpu_cells_limits as model  # noqa: E402

P_MAX = 17
MAX_NODES = 2000
N_TREE = {"flat": 300, "grid": 700}
BUDGETS = (1, 63, 64, 65, 200, 1000)
SEED, PID0 = 13, 500
FLAGS = (0, capi.DEBUG_CELLS_NO_PACING)
# every (P, split) pair in the benchmark's space (R^3, a grid); the other spaces and trees take one pair per P and per split
PAIRS_ALL = [(P, split) for P in (1, 3, 9, 17) for split in (1, 2, 3, 4, 8)]
PAIRS_FEW = [(1, 8), (3, 3), (9, 2), (17, 4), (17, 1)]
SHAPES = [(3, "grid", P, s) for P, s in PAIRS_ALL] + [(d, t, P, s) for d, t in ((3, "flat"), (2, "grid"), (2, "flat")) for P, s in PAIRS_FEW]


def _scene(dim):
    rng = np.random.default_rng(5100 + dim)
    c = rng.random((64, dim)) * 10.0
    r = 0.6 + rng.random(64) * (0.7 if dim == 3 else 0.2)
    return dict(dim=dim, bounds=[(0.0, 10.0)] * dim, max_distance=0.5, goal_bias=0.05, lvs_fraction=0.05, start=[1.0] * dim,
                goal_centre=[9.0] * dim, goal_radius=0.3, spheres=(c, r), boxes=None)


def _trees(dim, tree):
    rng = np.random.default_rng(5200 + dim + N_TREE[tree])
    out = []
    for _ in range(P_MAX):
        s, par = model._random_tree(rng, N_TREE[tree], 0.0, 10.0, dim)
        s[0] = 1.0
        out.append((s, par))
    level = model.cells_level(N_TREE[tree], dim, model.cells_level_max(dim, MAX_NODES))
    assert (level == 0) == (tree == "flat")
    return out


def _counts(o):
    return dict(nodes=o.num_nodes, iterations=o.iterations, accepted=o.accepted, checksum=o.checksum)


_WANT = {}


def _want(dim, tree, legs, pid0=PID0):
    """the oracle's counts of problems pid0 .. pid0 + 16 after every leg: a problem's results do not depend on the batch around
    it, so every P shares them"""
    key = (dim, tree, legs, pid0)
    if key not in _WANT:
        sc = _scene(dim)
        planners = [model._oracle(sc, SEED, pid0 + p, MAX_NODES, False) for p in range(P_MAX)]
        for o, (s, par) in zip(planners, _trees(dim, tree)):
            assert o.set_tree(s, par) == 0
        out = []
        for iters, freeze in legs:
            orc.solve_many(planners, iters, freeze=freeze, threads=4)
            out.append([_counts(o) for o in planners])
        if any(freeze for _, freeze in legs):   # non-vacuity: the frozen legs both accept and reject
            acc = sum(w["accepted"] for w in out[-1])
            assert 0.1 * sum(w["iterations"] for w in out[-1]) <= acc <= 0.9 * sum(w["iterations"] for w in out[-1])
        _WANT[key] = out
    return _WANT[key]


def _batch(dim, tree, P, split, flags, stamped=False, pid0=PID0):
    g = model._gpu(_scene(dim), P, MAX_NODES, False, SEED, pid0, stamped=stamped, frozen_split=split, debug_flags=flags)
    for p, (s, par) in enumerate(_trees(dim, tree)[:P]):
        g.set_tree(p, s, par)
    return g


def _step(g, P, iters, freeze, want, what):
    g.solve(iters, freeze=freeze)
    assert g.last_timing()["kernel"] == capi.KERNEL_CELLS
    c = g.counts()
    for p in range(P):
        got = {k: int(c[k][p]) for k in ("nodes", "iterations", "accepted", "checksum")}
        assert got == want[p], (what, p)
    return c


def _quota(P, budget, split):
    return P * int(capi.lib().oxhip_cells_problem_quota((budget + 63) // 64, split))


@pytest.mark.parametrize("dim,tree,P,split", SHAPES, ids=lambda v: str(v))
def test_budgets_in_a_row(dim, tree, P, split):
    """six frozen launches on one batch, budgets 1 .. 1000: both boards, each cleared by the launch before it"""
    legs = tuple((b, True) for b in BUDGETS)
    want = _want(dim, tree, legs)
    got = []
    for flags in FLAGS:
        g = _batch(dim, tree, P, split, flags)
        for i, (iters, freeze) in enumerate(legs):
            c = _step(g, P, iters, freeze, want[i], (flags, i, iters))
        got.append({k: c[k].copy() for k in ("iterations", "nodes", "accepted", "checksum")})
        g.close()
    for k in got[0]:
        assert np.array_equal(got[0][k], got[1][k]), k


@pytest.mark.parametrize("flags", FLAGS, ids=["paced", "no_pacing"])
def test_two_batches_stepped_alternately(flags):
    """each batch has boards and a parity of its own"""
    legs = ((200, True), (65, True), (1000, True), (64, True))
    want_a, want_b = _want(3, "grid", legs), _want(2, "flat", legs, PID0 + 100)
    a, b = _batch(3, "grid", 17, 3, flags), _batch(2, "flat", 9, 4, flags, pid0=PID0 + 100)
    for i, (iters, freeze) in enumerate(legs):
        _step(a, 17, iters, freeze, want_a[i], ("a", i))
        _step(b, 9, iters, freeze, want_b[i], ("b", i))
    a.close()
    b.close()


@pytest.mark.parametrize("flags", FLAGS, ids=["paced", "no_pacing"])
@pytest.mark.parametrize("split", [1, 3, 8])
def test_growing_launch_between_frozen_ones(split, flags):
    """the growing launch leaves the boards and the parity alone (and a tree that grew past the flat list gets its grid)"""
    legs = ((200, True), (400, False), (200, True), (65, True))
    want = _want(3, "flat", legs)
    assert want[1][0]["nodes"] > N_TREE["flat"]
    g = _batch(3, "flat", 9, split, flags)
    for i, (iters, freeze) in enumerate(legs):
        _step(g, 9, iters, freeze, want[i], (split, i))
    g.close()


@pytest.mark.parametrize("stamped", [False, True], ids=["product_build", "stamped_build"])
def test_goal_already_reached(stamped):
    """stop_at_goal with problems that have reached their goal: their waves leave right after the launch's barrier -- and
    report their whole quota on the way, so the board still ends at the live problems' quota"""
    dim, P, split = 3, 9, 3
    sc = dict(_scene(dim), spheres=None, goal_centre=[2.5] * dim, goal_radius=0.5, goal_bias=0.3)
    planners = [model._oracle(sc, SEED, PID0 + p, MAX_NODES, True) for p in range(P)]
    orc.solve_many(planners, 6, threads=4)
    reached = [o.goal_node >= 0 for o in planners]
    assert any(reached) and not all(reached), reached    # waves that leave early next to waves that run
    orc.solve_many(planners, 200, freeze=True, threads=4)
    want = [_counts(o) for o in planners]
    for flags in FLAGS:
        g = model._gpu(sc, P, MAX_NODES, True, SEED, PID0, stamped=stamped, frozen_split=split, debug_flags=flags)
        g.solve(6)
        c = _step(g, P, 200, True, want, flags)
        assert [int(v) >= 0 for v in c["goal_node"]] == reached
        if stamped:
            assert int(g.stamps()[capi.STAMP_CELLS_BOARD]) == _quota(P, 200, split)
        g.close()


@pytest.mark.parametrize("dim,tree,P,split", [(3, "grid", 17, 3), (3, "grid", 1, 8), (2, "flat", 9, 4), (3, "flat", 3, 1)], ids=lambda v: str(v))
def test_board_ends_at_the_quota(dim, tree, P, split):
    """the stamped build: after every frozen launch its board holds, over the XCDs, every live problem's quota -- whichever
    board it was, and whatever the launches before left on it"""
    legs = ((200, True), (65, True), (1000, True), (1, True))
    want = _want(dim, tree, legs)
    for flags in FLAGS:
        g = _batch(dim, tree, P, split, flags, stamped=True)
        for i, (iters, freeze) in enumerate(legs):
            _step(g, P, iters, freeze, want[i], (flags, i))
            assert int(g.stamps()[capi.STAMP_CELLS_BOARD]) == _quota(P, iters, split), (flags, i)
        g.close()
