"""The dealt pass of the cell-grid walk (rrt_cells.hip), restated in numpy and held against the plain walk.

After the first trip of a round (own cell + the nearer face cell per axis) the 64 lanes of a wave still ask for some of the
other cells of their 3^D blocks, very unevenly.  The kernel deals these (query, cell) pairs across the lanes: a prefix sum
over the lanes' counts places them in a list, lane k takes the pairs k, k + 64, ... up to DEPTH of them, and the owners get
the results back -- through an owner loop over per-pair lists, or through LDS atomics on two per-owner slots.  When the pairs
do not fit 64 x DEPTH, one ordinary trip runs first (every lane visits its next NB cells and re-prunes), then the rest is dealt.

`Wave.dealt` is that rule, wave-wide, with both merges; `plain_walk` is one lane on its own: visit every needed cell in order,
push every node into one (s1, s2, i1).  They share the geometry (`needed`), nothing of the placement or the merging.  Checked:
equal (s1, s2) always, equal i1 whenever s1 < s2 (on an exact tie the atomic merge may name the other node: such a query
fails the margin clause and is settled exactly).  The last test prints the distribution of pairs per round in the benchmark's
scene at 10,000 nodes: the capacity of 192 is chosen from it."""
import numpy as np
import pytest

from oracle import oracle_py as orc
from oxmpl_amd import scenarios

F = np.float32
INF = F(np.inf)
NONE = 0xFFFFFFFF
A = 1.0e-5                      # the screen's error bound in cell units (any small positive value serves the model)
ORDER3 = (12, 14, 10, 16, 4, 22, 9, 11, 15, 17, 3, 5, 21, 23, 1, 7, 19, 25, 0, 2, 6, 8, 18, 20, 24, 26)   # faces, edges, corners


def push(t, s, i):
    """top2_push: strict '<' names the holder, the second value is the median of three"""
    s1, s2, i1 = t
    if s < s1:
        i1 = i
    s2 = sorted((s, s1, s2))[1]
    return (min(s1, s), s2, i1)


def bits(s):
    return int(np.asarray(s, dtype=F).view(np.uint32))


def unbits(b):
    return np.asarray(b, dtype=np.uint32).view(F)[()]


class Grid:
    """nodes in cell units, filed by cell in index order; a cell of more than seven nodes is a chain of blocks, evaluated whole"""

    def __init__(self, pos, G):
        self.G = G
        self.pos = np.asarray(pos, dtype=F)
        self.cells = {}
        for i, c in enumerate(np.minimum(np.floor(self.pos).astype(int), G - 1)):
            self.cells.setdefault(tuple(c), []).append(i)

    def eval_cell(self, c, tq):
        """(s1, s2, i1) of one cell against a query, binary32, x then y then z"""
        t = (INF, INF, NONE)
        for i in self.cells.get(tuple(c), ()):
            e = self.pos[i] - tq
            t = push(t, F(F(F(e[0] * e[0]) + F(e[1] * e[1])) + F(e[2] * e[2])), i)
        return t


def thr_of(s1):
    if not s1 < INF:
        return INF
    d = np.sqrt(np.float64(s1)) * (1.0 + 2.0 ** -20) + 2.0 * A
    return np.nextafter(F(d * d * (1.0 + 2.0 ** -20)), INF)


def neighbour(cq, b):
    o = ORDER3[b]
    return (cq[0] + o % 3 - 1, cq[1] + (o // 3) % 3 - 1, cq[2] + o // 9 - 1)


def needed(grid, tq, cq, thr):
    """neighbour numbers (ORDER3) whose box comes within sqrt(thr) of the query; none outside the grid"""
    lo = [F(max(tq[k] - F(cq[k]), F(0))) ** 2 if cq[k] > 0 else INF for k in range(3)]
    hi = [F(max(F(cq[k] + 1) - tq[k], F(0))) ** 2 if cq[k] + 1 < grid.G else INF for k in range(3)]
    th = min(thr, np.finfo(F).max)
    out = []
    for b, o in enumerate(ORDER3):
        d = (o % 3 - 1, (o // 3) % 3 - 1, o // 9 - 1)
        l = F(0)
        for k in range(3):
            if d[k]:
                l = F(l + (lo[k] if d[k] < 0 else hi[k]))
        if not l > th:
            out.append(b)
    return out


def first_trip(grid, tq):
    """own cell and the nearer face cell along every axis: (cq, running pair, neighbour numbers still asked for)"""
    cq = tuple(int(min(max(np.floor(x), 0), grid.G - 1)) for x in tq)
    t = grid.eval_cell(cq, tq)
    done = set()
    for a in range(3):
        up = F(cq[a] + 1) - tq[a] < tq[a] - F(cq[a])
        if (cq[a] + 1 < grid.G) if up else (cq[a] > 0):
            b = 2 * a + (1 if up else 0)          # faces come first in ORDER3: -x +x -y +y -z +z
            done.add(b)
            t2 = grid.eval_cell(neighbour(cq, b), tq)
            t = push(push(t, t2[0], t2[2]), t2[1], NONE)
    need = [b for b in needed(grid, tq, cq, thr_of(t[0])) if b not in done]
    return cq, t, need


def plain_walk(grid, tq, cq, t, need, trips, nb):
    """one lane on its own: `trips` ordinary trips (nb cells, then re-prune), then every cell still needed, node by node"""
    need = list(need)
    for _ in range(trips):
        for b in need[:nb]:
            for i in grid.cells.get(neighbour(cq, b), ()):
                e = grid.pos[i] - tq
                t = push(t, F(F(F(e[0] * e[0]) + F(e[1] * e[1])) + F(e[2] * e[2])), i)
        keep = set(needed(grid, tq, cq, thr_of(t[0])))
        need = [b for b in need[nb:] if b in keep]
    for b in need:
        for i in grid.cells.get(neighbour(cq, b), ()):
            e = grid.pos[i] - tq
            t = push(t, F(F(F(e[0] * e[0]) + F(e[1] * e[1])) + F(e[2] * e[2])), i)
    return t


class Wave:
    def __init__(self, grid, queries):
        self.grid = grid
        self.tq = [np.asarray(q, dtype=F) for q in queries]
        self.lanes = [first_trip(grid, q) for q in self.tq]

    def pairs(self):
        return sum(len(n) for _, _, n in self.lanes)

    def dealt(self, nb, depth, early, merge):
        """the kernel's neighbour loop: returns the lanes' (s1, s2, i1) and the ordinary trips that ran before the deal"""
        grid, cq = self.grid, [l[0] for l in self.lanes]
        t = [l[1] for l in self.lanes]
        need = [list(l[2]) for l in self.lanes]
        trips = 0
        while any(need):
            total = sum(len(n) for n in need)
            if (early or trips) and total <= 64 * depth:
                first = np.concatenate([[0], np.cumsum([len(n) for n in need])])   # exclusive prefix sum over the lanes
                plist = [None] * total
                for lane in range(len(need)):
                    for j, b in enumerate(need[lane]):
                        plist[first[lane] + j] = (lane, b)
                res = [None] * total
                if merge == "atomic":
                    best = [(bits(x[0]) << 32) | x[2] for x in t]
                    second = [bits(x[1]) for x in t]
                for u in range(depth):
                    for k in range(64):                    # lane k takes pair k + 64 u
                        at = k + 64 * u
                        if at >= total:
                            break
                        o, b = plist[at]
                        r = grid.eval_cell(neighbour(cq[o], b), self.tq[o])
                        if merge == "atomic":
                            pk = (bits(r[0]) << 32) | r[2]
                            was, best[o] = best[o], min(best[o], pk)
                            second[o] = min(second[o], max(was, pk) >> 32, bits(r[1]))
                        else:
                            res[at] = r
                for lane in range(len(need)):
                    if merge == "atomic":
                        t[lane] = (unbits(best[lane] >> 32), unbits(second[lane]), best[lane] & 0xFFFFFFFF)
                    else:
                        for j in range(len(need[lane])):
                            r = res[first[lane] + j]
                            t[lane] = push(push(t[lane], r[0], r[2]), r[1], NONE)
                break
            trips += 1
            for lane in range(len(need)):
                for b in need[lane][:nb]:
                    r = grid.eval_cell(neighbour(cq[lane], b), self.tq[lane])
                    t[lane] = push(push(t[lane], r[0], r[2]), r[1], NONE)
                keep = set(needed(grid, self.tq[lane], cq[lane], thr_of(t[lane][0])))
                need[lane] = [b for b in need[lane][nb:] if b in keep]
        return t, trips

    def check(self, nb=3, depth=None, early=True):
        depth = nb if depth is None else depth
        out = {}
        for merge in ("owner", "atomic"):
            got, trips = self.dealt(nb, depth, early, merge)
            for lane, (cq, t0, need) in enumerate(self.lanes):
                want = plain_walk(self.grid, self.tq[lane], cq, t0, need, trips, nb)
                g = got[lane]
                assert bits(g[0]) == bits(want[0]) and bits(g[1]) == bits(want[1]), (merge, lane, g, want)
                if want[0] < want[1]:
                    assert g[2] == want[2], (merge, lane, g, want)
            out[merge] = trips
        assert out["owner"] == out["atomic"]
        return out["owner"]


def _random_grid(rng, n, G):
    return Grid(rng.random((n, 3)) * G, G)


def test_random_trees_both_merges():
    rng = np.random.default_rng(1)
    for G, n in ((6, 300), (8, 1200), (11, 1500)):
        grid = _random_grid(rng, n, G)
        for _ in range(3):
            w = Wave(grid, rng.random((64, 3)) * G)
            w.check(nb=3)
            w.check(nb=4)
            w.check(nb=3, depth=1, early=False)      # the walk as it was: one pair per lane, only after a trip


def test_nobody_asks():
    """a node on top of every query: d1 = 0, the bound 2A reaches no neighbour: the loop body never runs"""
    rng = np.random.default_rng(2)
    q = (rng.integers(0, 8, (64, 3)) + 0.5).astype(F)
    w = Wave(Grid(q, 8), q)
    assert w.pairs() == 0 and w.check() == 0


def test_one_lane_asks_for_23():
    """63 queries sit on nodes, one finds its first trip empty and asks for all 23 other cells, in an interior cell"""
    rng = np.random.default_rng(3)
    q = (rng.integers(0, 2, (64, 3)) + 0.5).astype(F)
    q[17] = (5.3, 5.4, 5.6)
    far = np.array([[4.2, 4.2, 4.2], [6.7, 6.1, 4.5], [6.5, 6.5, 6.5]], dtype=F)      # corner cells of the block only
    w = Wave(Grid(np.vstack([q[:17], q[18:], far]), 8), q)
    assert [len(l[2]) for l in w.lanes][17] == 23 and w.pairs() == 23
    assert w.check() == 0


def _wave_with_total(rng, total, G=12):
    """queries whose pairs sum to exactly `total`: lanes asking for 23 (empty first trip, interior cell) and lanes asking for
    nothing (a node on the query), topped up by one lane at the grid's corner, where fewer neighbours exist"""
    full, rest = divmod(total, 23)
    nodes, q = [], []
    for j in range(full):
        c = np.array([1 + 3 * (j % 3), 1 + 3 * ((j // 3) % 3), 1 + 3 * (j // 9)])
        q.append(c + np.array([0.3, 0.4, 0.6]))
        nodes.append(c + np.array([1.2, 1.2, 1.2]))          # a corner cell of its block
    grid_nodes = np.array(nodes, dtype=F)
    w = None
    for _ in range(2000):
        extra = rng.random((64 - full, 3)) * G
        qq = np.vstack([np.array(q).reshape(-1, 3), extra]).astype(F)
        pos = np.vstack([grid_nodes.reshape(-1, 3), extra[1:].astype(F)])   # every extra lane but the first sits on a node
        w = Wave(Grid(pos, G), qq)
        if w.pairs() == total:
            return w
    pytest.fail("no wave with %d pairs found" % total)
    return w


@pytest.mark.parametrize("nb", [3, 4])
def test_exactly_the_capacity_and_one_more(nb):
    rng = np.random.default_rng(4)
    fits = _wave_with_total(rng, 64 * nb)
    assert fits.check(nb=nb) == 0                      # dealt at once
    over = _wave_with_total(rng, 64 * nb + 1)
    assert over.check(nb=nb) == 1                      # one ordinary trip, then the deal


def test_exact_ties_across_two_cells():
    """two nodes mirrored across a cell face, bit-identical distances from the query, which neither cell is the first trip's:
    s1 == s2 under both merges (the named node may differ, which the margin clause makes harmless)"""
    G = 8
    q = np.full((64, 3), 3.5, dtype=F)
    q[:, 0] = 3.25                                       # nearer face along x: the -x cell; the pair lies across the +y / -y faces ...
    q[:, 1] = 3.5                                        # ... equally far: up = (hi < lo) is false, the first trip takes -y
    pos = np.array([[3.25, 4.25, 3.5], [3.25, 2.75, 3.5], [3.25, 4.25, 3.5], [7.5, 7.5, 7.5]], dtype=F)
    w = Wave(Grid(pos, G), q)
    got, _ = w.dealt(3, 3, True, "atomic")
    assert all(bits(g[0]) == bits(g[1]) for g in got)
    w.check()
    # ... and with both cells dealt: the pair across +x+y / +x-y edges
    pos2 = np.array([[4.125, 4.25, 3.5], [4.125, 2.75, 3.5], [0.5, 0.5, 0.5]], dtype=F)
    q2 = np.tile(np.array([3.75, 3.5, 3.5], dtype=F), (64, 1))
    w2 = Wave(Grid(pos2, G), q2)
    assert all(len(l[2]) >= 2 for l in w2.lanes)
    got2, _ = w2.dealt(3, 3, True, "atomic")
    assert all(bits(g[0]) == bits(g[1]) and g[0] < INF for g in got2)
    w2.check()


def test_cells_of_more_than_seven_nodes():
    rng = np.random.default_rng(6)
    G = 6
    pos = np.vstack([rng.random((400, 3)) * G] + [c + rng.random((19, 3)) for c in ((2, 2, 2), (3, 2, 2), (2, 3, 3), (4, 4, 4))])
    grid = Grid(pos, G)
    assert max(len(v) for v in grid.cells.values()) > 14
    for _ in range(3):
        Wave(grid, 1.5 + rng.random((64, 3)) * 3.0).check()


def test_pairs_per_round_in_the_benchmark_scene(capsys):
    """the benchmark's sphere field, a tree grown to 10,000 nodes by the oracle, the grid the kernel files it in (G = 16), 150
    rounds of 64 queries (5 % goal samples): pairs outstanding after the first trip.  The kernel's own stamps of the steady
    launch give 160.8 cells asked for per round (profiles/frozen_pacing/inkernel_stamps.txt); the model that chose the capacity
    gave a standard deviation of 22.  The bounds below are that measurement with five standard errors of 150 rounds around it,
    and the share of rounds within 192 pairs that a normal distribution of that mean and deviation gives (0.92), again less five
    standard errors.  This model finds mean 163.3, sd 21.0, 88 % of rounds within 192 pairs and all within 256 -- fewer rounds
    fit than the 97 % the capacity was first argued from; the others run one ordinary trip before the deal."""
    sc = scenarios.config2()
    o = orc.OracleRRT(sc["dim"], sc["bounds"], sc["max_distance"], sc["goal_bias"], sc["lvs_fraction"], 10000, False, 42, 0)
    o.set_spheres(*sc["spheres"])
    o.setup(sc["start"], sc["goal_centre"], sc["goal_radius"])
    o.solve(10 ** 7)
    states, _ = o.tree()
    assert states.shape[0] == 10000
    b = np.asarray(sc["bounds"], dtype=np.float64).reshape(3, 2)
    gc = np.asarray(sc["goal_centre"], dtype=np.float64)
    lo = np.minimum(np.minimum(b[:, 0], gc), states.min(axis=0))
    hi = np.maximum(np.maximum(b[:, 1], gc), states.max(axis=0))
    G = 16
    inv_h = G / float((hi - lo).max())
    grid = Grid((states - lo) * inv_h, G)
    rng = np.random.default_rng(7)
    totals, asking, fullest = [], [], []
    for _ in range(150):
        q = b[:, 0] + rng.random((64, 3)) * (b[:, 1] - b[:, 0])
        q[rng.random(64) < sc["goal_bias"]] = gc
        counts = [len(first_trip(grid, np.asarray((x - lo) * inv_h, dtype=F))[2]) for x in q]
        totals.append(sum(counts))
        asking.append(sum(1 for c in counts if c))
        fullest.append(max(counts))
    totals = np.array(totals)
    with capsys.disabled():
        print("\npairs outstanding after the first trip, 150 rounds: mean %.1f, sd %.1f, min %d, max %d; lanes asking %.1f; fullest lane "
              "mean %.1f, max %d; rounds within 128 / 192 / 256 pairs: %.0f %% / %.0f %% / %.0f %%"
              % (totals.mean(), totals.std(), totals.min(), totals.max(), np.mean(asking), np.mean(fullest), max(fullest),
                 100.0 * (totals <= 128).mean(), 100.0 * (totals <= 192).mean(), 100.0 * (totals <= 256).mean()))
    assert abs(totals.mean() - 160.8) <= 5.0 * 22.0 / np.sqrt(150.0)
    assert (totals <= 192).mean() >= 0.92 - 5.0 * np.sqrt(0.92 * 0.08 / 150.0)
    assert (totals <= 256).all()
