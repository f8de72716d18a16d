"""-m gpu: ambiguous queries of FROZEN cell-grid launches (rrt_cells.hip), against the oracle bit for bit.

A frozen round commits all its lanes; a lane whose screen cannot prove its nearest node is settled in place after the
round's commit -- among the nodes within the walk's pruning bound (the band resolver) or, when that declines, over the
whole tree -- and its term joins the round's checksum sum.  The scenes force the ambiguity through the goal sample: with
goal_bias 0.5 half of all queries are the goal centre, and the trees handed in (set_tree) hold two nodes at bit-identical
distance from it (a genuine tie: the lower index must win, rrt.rs:192) or at distances that differ by far less than the
screen's error bound 2A (the nearer node must win whatever its index).  The pair lies in one cell, in two cells across a
face, or with one node in the overflow block of a cell of 13 nodes.

OXHIP_DEBUG_SHORT_MEMO keeps a frozen launch from memoizing an answer, so every goal sample of a round is settled afresh:
several band settlements per round.  The declining paths: a band that reaches past the 3^D block (a pair 2.6 cells away in
an emptied region), more than 64 nodes in the band (200 nodes within 10^-6 of one sphere around the goal centre), and
OXHIP_DEBUG_ALL_WHOLE_TREE.  The stamped instantiation's counters ([14] band settlements, [54] ambiguous events, [53] lanes
offered minus iterations run) show the intended path was taken and that no lane is offered twice."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oxmpl_amd import capi, scenarios  # noqa: E402
from oracle import oracle_py as orc  # noqa: E402
import test_gpu_cells_limits as model  # noqa: E402

W_BAND, W_EXCESS, W_AMB, W_MEMO, W_TIE = 14, 53, 54, 55, 15
SPLITS = (1, 2, 3, 8)
ITERS = 448          # seven rounds: with 8 parts one part has no round
P = 4
MAX_NODES = 4000
N_BACKGROUND = {2: 1000, 3: 1400}   # beyond the brute list's 512: G = 23 (R^2) / 8 (R^3), about two nodes per cell


def _scene(dim, goal_centre):
    return dict(dim=dim, bounds=[(0.0, 10.0)] * dim, max_distance=0.5, goal_bias=0.5, lvs_fraction=0.05, start=[1.0] * dim,
                goal_centre=list(goal_centre), goal_radius=0.3,
                spheres=(np.array([[2.5] * dim, [7.5] + [2.5] * (dim - 1)]), np.array([0.9, 0.7])), boxes=None)


def _cell_width(dim, n):
    G = model.cells_G(model.cells_level(n, dim, model.cells_level_max(dim, MAX_NODES)))
    return 10.0 / G, G


def _dyadic(x, bits):
    return np.round(np.asarray(x, dtype=np.float64) * 2.0 ** bits) / 2.0 ** bits


def _pair_tree(rng, dim, kind, tie, reach=0.1):
    """(goal centre, states, parents): a random tree in [0, 10]^D with nothing nearer to the goal centre than the pair.  The
    goal centre lies on a 2^-10 lattice and the pair's offsets on a 2^-20 lattice, so mirror images are equally far bit for bit.
    `reach`: the pair's distance along axis 0, in cells."""
    n_bg = N_BACKGROUND[dim]
    h, G = _cell_width(dim, n_bg)
    cell = np.full(dim, G // 2)
    c = (cell + 0.5) * h
    if kind != "same_cell":
        c[0] = cell[0] * h                       # on the face between cell[0] - 1 and cell[0]
    c = _dyadic(c, 10)
    off = _dyadic(np.array([reach * h] + [0.05 * h] * (dim - 1)), 20)
    flip = np.array([-1.0] + [1.0] * (dim - 1))
    n1, n2 = c + off, c + off * flip             # n2: the mirror image below the face
    if tie == "near":
        n2 = n2 - np.array([1.0e-7] + [0.0] * (dim - 1))     # farther by ~10^-7: far inside 2A (~10^-5), not equal
    r = float(np.sqrt(((n2 - c) ** 2).sum()))
    bg = rng.random((n_bg, dim)) * 10.0
    bg = bg[np.sqrt(((bg - c) ** 2).sum(axis=1)) > r + 0.25 * h]
    bg[0] = 1.0
    if kind == "overflow":
        # twelve nodes in n2's cell, farther from the goal centre, at low indices: n2 is the cell's 13th entry (second block)
        fill = np.tile(c, (12, 1))
        fill[:, 0] = c[0] - (0.6 + 0.03 * np.arange(12)) * h
        fill[:, 1:] += (rng.random((12, dim - 1)) - 0.5) * 0.4 * h
        bg = np.vstack([bg[:1], fill, bg[1:]])
        pair = [n2, n1]                          # the node in the overflow block holds the lower index
    else:
        pair = [n1, n2]
    states = np.vstack([bg] + pair)
    n = states.shape[0]
    assert _cell_width(dim, n)[1] == G and n > model.BRUTE
    lo, inv_h, gk = model.grid_of(states, n, [(0.0, 10.0)] * dim, c, MAX_NODES)
    ca, cb = model.cell_of(pair[0], lo, inv_h, gk), model.cell_of(pair[1], lo, inv_h, gk)
    if kind == "same_cell":
        assert (ca == cb).all() and (ca == model.cell_of(c, lo, inv_h, gk)).all()
    elif reach < 1.0:
        assert abs(int(ca[0]) - int(cb[0])) == 1 and (ca[1:] == cb[1:]).all()
    if kind == "overflow":
        cells = model.cell_of(states, lo, inv_h, gk)
        assert int((cells[:n - 2] == ca).all(axis=1).sum()) >= 12    # n2 is at best the cell's 13th entry
    d = np.sqrt(((states - c) ** 2).sum(axis=1))
    if tie == "exact":
        assert d[n - 2] == d[n - 1] == d.min()
    else:
        assert d[n - 2] != d[n - 1] and abs(d[n - 2] - d[n - 1]) < 2.0e-7 and d[:n - 2].min() > max(d[n - 2], d[n - 1])
    parents = np.concatenate([[-1], rng.integers(0, np.arange(1, n))]).astype(np.int32)
    return c, states, parents


def _want(sc, trees, seed, pid0, iters):
    planners = [model._oracle(sc, seed, pid0 + p, MAX_NODES, False) for p in range(len(trees))]
    for o, (s, par) in zip(planners, trees):
        assert o.set_tree(s, par) == 0
    orc.solve_many(planners, iters, freeze=True, threads=4)
    return [model._snap(o) for o in planners]


def _run(sc, trees, seed, pid0, iters, want, stamped=False, **extra):
    gpu = model._gpu(sc, len(trees), MAX_NODES, False, seed, pid0, stamped=stamped, **extra)
    for p, (s, par) in enumerate(trees):
        gpu.set_tree(p, s, par)
    gpu.solve(iters, freeze=True)
    assert gpu.last_timing()["kernel"] == capi.KERNEL_CELLS
    c = gpu.counts()
    for p in range(len(trees)):
        model._same(gpu, p, want[p], c, (p, extra))
    s = gpu.stamps() if stamped else None
    gpu.close()
    return s


def _pair_case(dim, kind, tie, seed, reach=0.1):
    rng = np.random.default_rng(seed)
    trees, c = [], None
    for _ in range(P):
        c, s, par = _pair_tree(rng, dim, kind, tie, reach)
        trees.append((s, par))
    sc = _scene(dim, c)
    return sc, trees


@pytest.mark.parametrize("tie", ["exact", "near"])
@pytest.mark.parametrize("kind", ["same_cell", "across_face", "overflow"])
@pytest.mark.parametrize("dim", [2, 3])
def test_goal_sample_ties_every_split(dim, kind, tie):
    """the same counters, checksums and trees for every split, all equal to the oracle's; the stamped run shows that the band
    resolver settled the queries, that the memo answered the repeats and that every lane offered was an iteration run"""
    sc, trees = _pair_case(dim, kind, tie, 9000 + 10 * dim + len(kind) + len(tie))
    want = _want(sc, trees, 5, 40, ITERS)
    for split in SPLITS:
        _run(sc, trees, 5, 40, ITERS, want, frozen_split=split)
    s = _run(sc, trees, 5, 40, ITERS, want, stamped=True, frozen_split=3)
    assert int(s[W_BAND]) >= P and int(s[W_AMB]) >= int(s[W_BAND]) and int(s[W_MEMO]) > 0.3 * P * ITERS, s[[W_BAND, W_AMB, W_MEMO]]
    assert int(s[W_EXCESS]) == 0


@pytest.mark.parametrize("tie", ["exact", "near"])
@pytest.mark.parametrize("dim", [2, 3])
def test_goal_sample_ties_without_memo(dim, tie):
    """OXHIP_DEBUG_SHORT_MEMO: no answer is kept, so each of a round's ~32 goal samples is settled by the band resolver"""
    sc, trees = _pair_case(dim, "overflow", tie, 9100 + dim + len(tie))
    want = _want(sc, trees, 6, 50, ITERS)
    for split in (1, 3):
        _run(sc, trees, 6, 50, ITERS, want, frozen_split=split, debug_flags=capi.DEBUG_SHORT_MEMO)
    s = _run(sc, trees, 6, 50, ITERS, want, stamped=True, frozen_split=2, debug_flags=capi.DEBUG_SHORT_MEMO)
    assert int(s[W_BAND]) > 0.3 * P * ITERS and int(s[W_MEMO]) == 0, s[[W_BAND, W_AMB, W_MEMO]]
    # (the goal samples never go to the whole-tree path; a uniform query is ambiguous 2 10^-4 of the time -- 0.2 expected among these
    #  ~900 -- and may then be declined)
    assert int(s[W_AMB]) - int(s[W_BAND]) <= 2
    assert int(s[W_EXCESS]) == 0


def test_no_lane_is_offered_twice():
    """lanes offered = iterations run while ambiguous queries were settled (before the in-place rule every ambiguous query cost
    the lanes behind it: 4132 lanes for 4096 iterations in the committed stamps of the benchmark shape)"""
    sc, trees = _pair_case(3, "across_face", "exact", 77)
    want = _want(sc, trees, 7, 60, ITERS)
    for split, flags in ((1, 0), (3, 0), (3, capi.DEBUG_SHORT_MEMO)):
        s = _run(sc, trees, 7, 60, ITERS, want, stamped=True, frozen_split=split, debug_flags=flags)
        assert int(s[W_AMB]) > 0 and int(s[W_EXCESS]) == 0, (split, flags, int(s[W_AMB]), int(s[W_EXCESS]))
        assert int(s[model.W_ITER0]) == ITERS


@pytest.mark.parametrize("tie", ["exact", "near"])
@pytest.mark.parametrize("dim", [2, 3])
def test_decline_band_reaches_past_the_block(dim, tie):
    """the pair 2.6 cells from the goal centre, nothing nearer: the shell search finds it, the margin fails, the band bound
    exceeds the block's open faces -- the resolver declines and the whole-tree path answers"""
    sc, trees = _pair_case(dim, "across_face", tie, 9200 + dim + len(tie), reach=2.6)
    want = _want(sc, trees, 8, 70, ITERS)
    for split in (1, 3):
        _run(sc, trees, 8, 70, ITERS, want, frozen_split=split)
    s = _run(sc, trees, 8, 70, ITERS, want, stamped=True, frozen_split=2, debug_flags=capi.DEBUG_SHORT_MEMO)
    assert int(s[W_AMB]) - int(s[W_BAND]) > 0.3 * P * ITERS and int(s[W_BAND]) <= 2, s[[W_BAND, W_AMB]]   # (<= 2: ambiguous uniform queries)
    assert int(s[model.W_SHELL]) > 0 and int(s[W_EXCESS]) == 0
    if tie == "exact":
        assert int(s[W_TIE]) > 0                 # (problem 0's literal loops)


@pytest.mark.parametrize("dim", [2, 3])
def test_decline_more_than_64_band_nodes(dim):
    """200 nodes on directions spread around the goal centre at radii within 10^-6 of each other (one cell, a chain of 29 blocks):
    far more than 64 of them inside the band"""
    rng = np.random.default_rng(9300 + dim)
    n_bg = N_BACKGROUND[dim]
    h, G = _cell_width(dim, n_bg)
    c = _dyadic((np.full(dim, G // 2) + 0.5) * h, 10)
    trees = []
    for _ in range(2):
        u = rng.normal(size=(200, dim))
        u /= np.sqrt((u * u).sum(axis=1))[:, None]
        ring = c + u * (0.2 * h + rng.random(200) * 1.0e-6)[:, None]
        bg = rng.random((n_bg, dim)) * 10.0
        bg = bg[np.sqrt(((bg - c) ** 2).sum(axis=1)) > 0.45 * h]
        bg[0] = 1.0
        states = np.vstack([bg, ring])
        n = states.shape[0]
        assert _cell_width(dim, n)[1] == G
        parents = np.concatenate([[-1], rng.integers(0, np.arange(1, n))]).astype(np.int32)
        trees.append((states, parents))
    sc = _scene(dim, c)
    want = _want(sc, trees, 9, 80, ITERS)
    for split in (1, 3):
        _run(sc, trees, 9, 80, ITERS, want, frozen_split=split)
    s = _run(sc, trees, 9, 80, ITERS, want, stamped=True, frozen_split=2, debug_flags=capi.DEBUG_SHORT_MEMO)
    assert int(s[W_AMB]) - int(s[W_BAND]) > 0.3 * 2 * ITERS and int(s[W_BAND]) <= 2, s[[W_BAND, W_AMB]]   # (<= 2: ambiguous uniform queries)
    assert int(s[W_EXCESS]) == 0


@pytest.mark.parametrize("stamped", [False, True], ids=["product_build", "stamped_build"])
def test_decline_all_whole_tree(stamped):
    """OXHIP_DEBUG_ALL_WHOLE_TREE on a frozen launch of 2 problems x 256 iterations: every lane of a round is ambiguous and
    is settled by the whole-tree path, one after the other; no band settlement, no lane offered twice"""
    sc, trees = _pair_case(3, "same_cell", "exact", 9400)
    trees = trees[:2]
    want = _want(sc, trees, 10, 90, 256)
    for split, flags in ((1, capi.DEBUG_ALL_WHOLE_TREE), (2, capi.DEBUG_ALL_WHOLE_TREE | capi.DEBUG_SHORT_MEMO)):
        s = _run(sc, trees, 10, 90, 256, want, stamped=stamped, frozen_split=split, debug_flags=flags)
        if stamped:
            assert int(s[W_BAND]) == 0 and int(s[W_EXCESS]) == 0
            assert int(s[W_AMB]) + int(s[W_MEMO]) >= 2 * 256, s[[W_AMB, W_MEMO]]
            if flags & capi.DEBUG_SHORT_MEMO:    # (no memo: every iteration is one whole-tree event)
                assert int(s[W_MEMO]) == 0 and int(s[W_AMB]) == 2 * 256


def test_growing_launch_is_unchanged_then_frozen():
    """a config2 batch of 8 problems grown to 1,500 nodes (the growing kernel keeps its cut and its whole-tree path), then 512
    frozen iterations: equal to the oracle at both points"""
    sc = scenarios.config2()
    n_p = 8
    gpu = scenarios.make_batch(sc, n_p, 1500, False, 42, 0, 0, capi.KERNEL_CELLS, frozen_split=3)
    planners = [model._oracle(sc, 42, p, 1500, False) for p in range(n_p)]
    gpu.solve(10 ** 6)
    orc.solve_many(planners, 10 ** 6, threads=4)
    c = gpu.counts()
    assert int(c["nodes"].min()) == 1500
    for p in range(n_p):
        model._same(gpu, p, model._snap(planners[p]), c, ("grown", p))
    gpu.solve(512, freeze=True)
    orc.solve_many(planners, 512, freeze=True, threads=4)
    c = gpu.counts()
    for p in range(n_p):
        model._same(gpu, p, model._snap(planners[p]), c, ("frozen", p))
    gpu.close()
