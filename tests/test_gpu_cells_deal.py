"""-m gpu: the dealt pass of the cell-grid walk (rrt_cells.hip, DESIGN.md 5.6 "The walk"), against the oracle bit for bit.

After a frozen round's first trip the outstanding (query, cell) pairs are dealt across the lanes, three deep, and merged into
per-owner slots; when they do not fit, ordinary trips run first.  Small trees handed in with set_tree (600 to 3,000 nodes: above
the flat list, grid levels G = 6 ... 11), frozen launches of 1 to 256 iterations -- budgets of 1, 63, 65 and 100 end in a round
with idle lanes -- with frozen_split 1 and 3, in R^3 and R^2.  Node counts, iteration counts, checksums and trees equal the
oracle's; on the stamped build problem 0's words [1] (dealt passes), [2] (pairs dealt) and the trip histogram [24 ...] show which
way the walk went.  The growing launch at the end shows the growing path computing what it did."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oxmpl_amd import capi  # noqa: E402
from oracle import oracle_py as orc  # noqa: E402
import test_gpu_cells_limits as model  # noqa: E402

W_DEALT, W_PAIRS, W_TRIP0, W_TRIP1, W_BAND, W_AMB = 1, 2, 24, 25, 14, 54
MAX_NODES = 4000
LEGS = (1, 63, 65, 100, 256)          # frozen launches, one after the other on one batch
SPLITS = (1, 3)
_WANT = {}


def _scene(dim, goal_centre=None, goal_bias=0.05, spheres=True):
    sph = (np.array([[2.5] * dim, [7.5] + [2.5] * (dim - 1)]), np.array([0.9, 0.7])) if spheres else None
    return dict(dim=dim, bounds=[(0.0, 10.0)] * dim, max_distance=0.5, goal_bias=goal_bias, lvs_fraction=0.05, start=[1.0] * dim,
                goal_centre=[9.0] * dim if goal_centre is None else list(goal_centre), goal_radius=0.3, spheres=sph, boxes=None)


def _want(key, sc, trees, seed, pid0):
    """the oracle's state after every frozen leg, once per case (splits and builds share it)"""
    if key not in _WANT:
        planners = [model._oracle(sc, seed, pid0 + p, MAX_NODES, False) for p in range(len(trees))]
        for o, (s, par) in zip(planners, trees):
            assert o.set_tree(s, par) == 0
        out = []
        for iters in LEGS:
            orc.solve_many(planners, iters, freeze=True, threads=4)
            out.append([model._snap(o) for o in planners])
        _WANT[key] = out
    return _WANT[key]


def _run(key, sc, trees, seed, pid0, split, stamped, flags=0):
    want = _want(key, sc, trees, seed, pid0)
    gpu = model._gpu(sc, len(trees), MAX_NODES, False, seed, pid0, stamped=stamped, frozen_split=split, debug_flags=flags)
    for p, (s, par) in enumerate(trees):
        gpu.set_tree(p, s, par)
    for i, iters in enumerate(LEGS):
        gpu.solve(iters, freeze=True)
        assert gpu.last_timing()["kernel"] == capi.KERNEL_CELLS
        c = gpu.counts()
        for p in range(len(trees)):
            model._same(gpu, p, want[i][p], c, (key, split, i, p))
    s = gpu.stamps() if stamped else None
    gpu.close()
    return s


def _tree(rng, n, lo, hi, dim):
    s, par = model._random_tree(rng, n, lo, hi, dim)
    s[0] = 1.0
    return s, par


BUILD = pytest.mark.parametrize("stamped", [False, True], ids=["product_build", "stamped_build"])
SPLIT = pytest.mark.parametrize("split", SPLITS)
DIM = pytest.mark.parametrize("dim", [2, 3])


@BUILD
@SPLIT
@DIM
def test_free_space_tree_is_dealt_after_the_first_trip(dim, split, stamped):
    """trees spread over the whole box, one to eight problems' worth of sizes: every round's pairs fit three per lane"""
    rng = np.random.default_rng(100 + dim)
    sizes = (600, 1100, 3000) if dim == 3 else (600, 1700, 3000)
    trees = [_tree(rng, n, 0.0, 10.0, dim) for n in sizes]
    s = _run(("free", dim), _scene(dim), trees, 11, 300, split, stamped)
    if stamped:
        assert int(s[W_DEALT]) > 0 and int(s[W_PAIRS]) > 0
        assert int(s[W_TRIP1]) == 0, "a third trip ran"


@BUILD
@SPLIT
@DIM
def test_corner_tree_runs_trips_before_the_deal(dim, split, stamped):
    """the tree fills one corner of the bounds at a density that makes the grid fine: most queries find their neighbourhood
    empty and ask for every cell of it -- far more than three pairs per lane"""
    rng = np.random.default_rng(200 + dim)
    trees = [_tree(rng, n, 0.0, 4.0, dim) for n in (2500, 900)]
    s = _run(("corner", dim), _scene(dim, spheres=False), trees, 12, 310, split, stamped)
    if stamped:
        assert int(s[W_TRIP0]) > 0, "no ordinary trip ran"
        assert int(s[W_DEALT]) > 0


@BUILD
@SPLIT
@DIM
def test_crowded_neighbour_cells_have_chains(dim, split, stamped):
    """clusters of 12 to 20 nodes inside single cells all over the box (as test_gpu_cells_limits crowds them, by position):
    the dealt cells carry overflow blocks"""
    rng = np.random.default_rng(300 + dim)
    trees = []
    for n_bg in (700, 1500):
        bg = rng.random((n_bg, dim)) * 10.0
        centres = rng.random((60, dim)) * 10.0
        cl = np.vstack([c + (rng.random((int(rng.integers(12, 21)), dim)) - 0.5) * 0.05 for c in centres])
        states = np.clip(np.vstack([bg, cl]), 0.0, 10.0)
        states[0] = 1.0
        n = states.shape[0]
        assert model.fullest_cell(states, n, [(0.0, 10.0)] * dim, [9.0] * dim, MAX_NODES) > 7
        trees.append((states, np.concatenate([[-1], rng.integers(0, np.arange(1, n))]).astype(np.int32)))
    s = _run(("crowded", dim), _scene(dim), trees, 13, 320, split, stamped)
    if stamped:
        assert int(s[W_DEALT]) > 0


@BUILD
@SPLIT
@DIM
def test_queries_on_faces_and_corners_of_the_bounds(dim, split, stamped):
    """half of the queries are the goal centre, which is a corner of the bounds (problems 0, 1) or lies on a face (2, 3) -- the
    scene has one goal, so two scenes; the other half is uniform in a grid of six to eleven cells, most of whose cells touch
    the boundary: neighbours outside the grid are never asked for"""
    rng = np.random.default_rng(400 + dim)
    for tag, gc in (("corner", [10.0] * dim), ("face", [10.0] + [5.0] * (dim - 1))):
        trees = [_tree(rng, n, 0.0, 10.0, dim) for n in (650, 2200)]
        s = _run(("bounds", tag, dim), _scene(dim, goal_centre=gc, goal_bias=0.5), trees, 14, 330, split, stamped)
        if stamped:
            assert int(s[W_DEALT]) > 0


def _tie_tree(rng, dim, tie):
    """two nodes mirrored through the goal centre's cell along axis 0 and shifted 0.6 cells along axis 1: they lie in two edge
    neighbours of the centre's cell, neither of which the first trip visits, at bit-identical (or nearly identical) distances;
    nothing else is as near"""
    n_bg = {2: 1000, 3: 1400}[dim]
    G = model.cells_G(model.cells_level(n_bg, dim, model.cells_level_max(dim, MAX_NODES)))
    h = 10.0 / G
    cell = np.full(dim, G // 2)
    c = np.round((cell + 0.5) * h * 2.0 ** 10) / 2.0 ** 10
    off = np.round(np.array([0.6 * h, 0.6 * h] + [0.05 * h] * (dim - 2)) * 2.0 ** 20) / 2.0 ** 20
    flip = np.array([-1.0] + [1.0] * (dim - 1))
    n1, n2 = c + off, c + off * flip
    if tie == "near":
        n2 = n2 - np.array([1.0e-7] + [0.0] * (dim - 1))
    r = float(np.sqrt(((n2 - c) ** 2).sum()))
    bg = rng.random((n_bg, dim)) * 10.0
    bg = bg[np.sqrt(((bg - c) ** 2).sum(axis=1)) > r + 0.25 * h]
    bg[0] = 1.0
    states = np.vstack([bg, n1, n2])
    n = states.shape[0]
    lo, inv_h, gk = model.grid_of(states, n, [(0.0, 10.0)] * dim, c, MAX_NODES)
    cc, ca, cb = (model.cell_of(x, lo, inv_h, gk) for x in (c, n1, n2))
    assert int(gk[0]) == G and n > model.BRUTE
    assert ca[0] == cc[0] + 1 and cb[0] == cc[0] - 1 and ca[1] == cb[1] == cc[1] + 1 and (ca[2:] == cc[2:]).all()
    d = np.sqrt(((states - c) ** 2).sum(axis=1))
    assert (d[n - 2] == d[n - 1]) if tie == "exact" else (d[n - 2] != d[n - 1] and abs(d[n - 2] - d[n - 1]) < 2.0e-7)
    assert d[:n - 2].min() > max(d[n - 2], d[n - 1])
    return c, (states, np.concatenate([[-1], rng.integers(0, np.arange(1, n))]).astype(np.int32))


@BUILD
@SPLIT
@pytest.mark.parametrize("tie", ["exact", "near"])
@DIM
def test_near_tie_across_two_dealt_cells_reaches_the_settlement(dim, tie, split, stamped):
    """every goal sample (half of all queries; OXHIP_DEBUG_SHORT_MEMO: each settled afresh) sees the pair through two dealt cells:
    the merge must hand the settlement code s1 with s2 within the margin, and the lower index (exact tie) or the nearer node wins"""
    rng = np.random.default_rng(500 + dim)
    c, t0 = _tie_tree(rng, dim, tie)
    trees = [t0, _tie_tree(rng, dim, tie)[1]]
    s = _run(("tie", dim, tie), _scene(dim, goal_centre=c, goal_bias=0.5), trees, 15, 340, split, stamped, flags=capi.DEBUG_SHORT_MEMO)
    if stamped:
        assert int(s[W_AMB]) > 0 and int(s[W_BAND]) > 0
        assert int(s[W_DEALT]) > 0


@BUILD
@DIM
def test_growing_launch_one_to_2000_nodes(dim, stamped):
    sc, P = _scene(dim), 2
    legs = [(1500, False), (10 ** 6, False)]
    want = model._oracle_legs(("deal_grow", dim), lambda: [model._oracle(sc, 16, 350 + p, 2000, False) for p in range(P)], legs, P)
    gpu = model._gpu(sc, P, 2000, False, 16, 350, stamped=stamped)
    model._run_legs(gpu, legs, want, P)
    assert int(gpu.counts()["nodes"].min()) == 2000
    gpu.close()
