"""Shapes for the RRT tree re-check (oxhip_rrt_batch_revalidate_trees, rrt_revalidate.hip) at the limits the
planted scenes of tests/rrt_revalidate_helpers.py do not reach:
  A  mixed     trees of very different sizes in one batch (R^3: 1, 2, 64, 257, 1024 = capacity, 65, 512, 1; SO(3): 1, 600, 130;
               SO(2): 1, 300, 1024): the per-problem guards of grids sized by the largest tree, the SO(3) staging chunks
  B  moves     R^2 trees of 1,024 / 1,025 nodes whose removed set is exactly a chosen index range: every survivor moves down by
               exactly 256, 255, 257, by half its index, by 1,023, by 1 -- the in-place compaction across tiles
  C  windows   R^3 and R^8, 63 / 64 / 65 / 128 / 129 spheres (and two boxes), a thin decisive sphere first, 64th, 65th or last of the
               table: the windows of 64 spheres of the edge kernel's midpoint filter
  D  steps     a child equal to its parent, half a resolution, dist / res at, one ulp below and one ulp above 1 and 2, a 2,000-step
               edge, a root inside an obstacle
  E  outside   nodes at -50, 1e3 and 1e5 with bounds [0, 10]^d (edges cut, far, grazed); a tree of A and one of B moved whole into
               translated, tiny and huge frames
  F  goal      distance == radius exactly and one ulp to either side; satisfying nodes in three tiles with the lowest ones removed
  G  twins     duplicate nodes whose lower twin dies, placed so that the skip kernel finds (or must not find) the twin in a later
               pass, another tile, the same wave
  H  rounds    (no planted shape: test_gpu_rrt_revalidate_limits.py moves obstacles round after round on grown trees)

A shape is a dict: name, space ("rn" | "so3" | "so2"), dim (row width: 4 on SO(3), 1 on SO(2)), bounds, fraction, max_nodes, trees
[(states [n][dim], parents [n])] (one per problem), goals [(centre, radius)], sph_c / sph_r (SO(3): cones), box_lo / box_hi (SO(2):
forbidden arcs).  Plain numpy and Python: nothing here loads the GPU library.  The verdicts are the references': the C oracle
(oracle/rrt_oracle.c through oracle_py.OracleRRT) over R^n, tests/golden/make_golden_so3.py over SO(3), make_golden_so2.py over
SO(2) -- `Ref`; survival, remapping and the goal node are the plain loops of rrt_revalidate_helpers.expected -- `reference`.  Thin
obstacles (radius 1e-9) sit on a state that the reference's check_motion tests: they cut that edge whatever the geometry around it.
Shapes and references are computed once and shared: never modify one.  tests/test_rrt_revalidate_limits_model.py holds every shape
to the property it exists for, and every edge to at most MAX_STEPS check steps (an edge of astronomic step count is one GPU
thread looping for minutes)."""
import functools
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden as mg  # noqa: E402
import make_golden_so2 as g2  # noqa: E402
import make_golden_so3 as g3  # noqa: E402

from oracle import oracle_py as orc  # noqa: E402
import rrt_revalidate_helpers as rh  # noqa: E402

FRACTION = 0.05
THIN = 1e-9
MAX_STEPS = 20000
SO3_BOUNDS = [0.0, 0.0, 0.0, 1.0, math.pi]
SO2_BOUNDS = [-g2.PI, g2.PI]
WIDTH = dict(so3=4, so2=1)


def shape(name, space, dim, trees, goals, sph=None, boxes=None, bounds=None, fraction=FRACTION, max_nodes=None, **extra):
    w = WIDTH.get(space, dim)
    sc, sr = sph if sph is not None else ([], [])
    bl, bh = boxes if boxes is not None else ([], [])
    if bounds is None:
        bounds = dict(rn=[(0.0, 10.0)] * dim, so3=SO3_BOUNDS, so2=SO2_BOUNDS)[space]
    trees = [(np.array(s, dtype=np.float64).reshape(-1, w), np.array(p, dtype=np.int32)) for s, p in trees]
    S = dict(name=name, space=space, dim=w, bounds=bounds, fraction=fraction, trees=trees,
             goals=[(np.array(c, dtype=np.float64).reshape(w), float(r)) for c, r in goals],
             max_nodes=max_nodes if max_nodes is not None else max(len(p) for _, p in trees) + 8,
             sph_c=np.array(sc, dtype=np.float64).reshape(-1, w), sph_r=np.array(sr, dtype=np.float64).reshape(-1),
             box_lo=np.array(bl, dtype=np.float64).reshape(-1, w), box_hi=np.array(bh, dtype=np.float64).reshape(-1, w))
    assert len(S["trees"]) == len(S["goals"]) and len(S["sph_c"]) == len(S["sph_r"]) and len(S["box_lo"]) == len(S["box_hi"])
    for s, p in trees:
        assert len(s) == len(p) <= S["max_nodes"] and p[0] == -1 and all(0 <= p[i] < i for i in range(1, len(p)))
        s.setflags(write=False)
        p.setflags(write=False)
    for a in ("sph_c", "sph_r", "box_lo", "box_hi"):
        S[a].setflags(write=False)
    S.update(extra)
    return S


def sizes(S):
    return [len(p) for _, p in S["trees"]]


# ============================================================================================================ the references
class Ref:
    """distance / num_steps / check_motion of the shape's space among its obstacles, by the reference implementations.
    without_sphere: that entry of the sphere table left out"""

    def __init__(self, S, without_sphere=None):
        self.S, self.space = S, S["space"]
        c, r = S["sph_c"], S["sph_r"]
        if without_sphere is not None:
            c, r = np.delete(c, without_sphere, axis=0), np.delete(r, without_sphere)
        if self.space == "so3":
            self.cones = g3.Cones([([float(v) for v in cc], float(rr)) for cc, rr in zip(c, r)])
        elif self.space == "so2":
            self.arcs = g2.Arcs([(float(lo[0]), float(hi[0])) for lo, hi in zip(S["box_lo"], S["box_hi"])])
        else:
            d = S["dim"]
            self.lvsl = orc.maximum_extent(S["bounds"]) * S["fraction"]
            self.o = orc.OracleRRT(d, S["bounds"], 1.0, 0.05, S["fraction"])
            if len(r):
                self.o.set_spheres(c, r)
            if len(S["box_lo"]):
                self.o.set_boxes(S["box_lo"], S["box_hi"])
            self.o.setup([0.0] * d, [0.0] * d, 0.0)

    def distance(self, a, b):
        if self.space == "so3":
            return g3.distance([float(v) for v in a], [float(v) for v in b])
        if self.space == "so2":
            return g2.distance(float(a[0]), float(b[0]))
        return orc.distance(a, b)

    def steps(self, a, b):
        if self.space == "so3":
            return mg.num_steps(self.distance(a, b), g3.lvsl(self.S["fraction"]))
        if self.space == "so2":
            return mg.num_steps(self.distance(a, b), g2.lvsl(self.S["fraction"]))
        return orc.num_steps(orc.distance(a, b), self.lvsl)

    def tested_state(self, a, b, k, n=None):
        """the k-th state that check_motion(a -> b) tests, k = 1 .. num_steps (to the bit: the reference's own interpolate)"""
        n = self.steps(a, b) if n is None else n
        assert 1 <= k <= n
        t = float(k) / float(n)
        if self.space == "so3":
            return np.array(g3.interpolate([float(v) for v in a], [float(v) for v in b], t))
        if self.space == "so2":
            return np.array([g2.interpolate(float(a[0]), float(b[0]), t)])
        return orc.interpolate(a, b, t)

    def check_motion(self, a, b):
        if self.space == "so3":
            return g3.check_motion(self.cones, self.S["fraction"], [float(v) for v in a], [float(v) for v in b])
        if self.space == "so2":
            return g2.check_motion(self.arcs, self.S["fraction"], float(a[0]), float(b[0]))
        return self.o.check_motion(a, b)


def resolution(S):
    """what check_motion divides the distance by: a tenth of the longest valid segment"""
    if S["space"] == "so3":
        return g3.lvsl(S["fraction"]) * 0.1
    if S["space"] == "so2":
        return g2.lvsl(S["fraction"]) * 0.1
    return orc.maximum_extent(S["bounds"]) * S["fraction"] * 0.1


_REFERENCES = {}


def reference(S, without_sphere=None):
    """per problem what the call must leave (rrt_revalidate_helpers.expected) plus sat (goal membership of every old node),
    goal_before, goal_lost, removed (the old indices that go) and max_steps"""
    key = (S["name"], without_sphere)
    if key not in _REFERENCES:
        ref, out = Ref(S, without_sphere), []
        for (st, par), (gc, gr) in zip(S["trees"], S["goals"]):
            n = len(par)
            ok = np.ones(n, dtype=bool)
            max_steps = 0
            for i in range(1, n):
                ok[i] = ref.check_motion(st[par[i]], st[i])
                max_steps = max(max_steps, int(ref.steps(st[par[i]], st[i])))
            sat = np.array([ref.distance(s, gc) <= gr for s in st], dtype=bool)
            e = rh.expected(st, par, ok, sat)
            e.update(sat=sat, goal_before=rh.goal_node(sat), max_steps=max_steps, removed=[i for i in range(n) if e["new_index"][i] < 0])
            e["goal_lost"] = e["goal_before"] >= 0 and e["goal_node"] < 0
            out.append(e)
        _REFERENCES[key] = out
    return _REFERENCES[key]


def counts(S):
    ref = reference(S)
    return "%-26s n %-40s removed %s" % (S["name"], sizes(S), [e["n_removed"] for e in ref])


# ============================================================================================================ trees
def move(space, rng, s, step):
    """a state at most about `step` from s"""
    if space == "so3":
        q = rh.quat_mul(s, rh.quat_axis_half(rng.normal(size=3), rng.uniform(0.3 * step, step)))
        return q / math.sqrt(float(q @ q))
    return s + rng.uniform(-step, step, size=len(s))


def near(space, a, b):
    """a construction-time distance (no verdict depends on it)"""
    if space == "so3":
        return math.acos(min(abs(float(a @ b)), 1.0))
    if space == "so2":
        return abs((float(a[0] - b[0]) + math.pi) % (2.0 * math.pi) - math.pi)
    return float(np.abs(a - b).max())


def bushy(space, n, root, seed, step, reach, leaves=()):
    """n states, every parent among the previous 40 nodes (never one of `leaves`), every edge at most about `step` long, every node
    within `reach` of the root (R^n: per coordinate)"""
    rng = np.random.RandomState(seed)
    root = np.array(root, dtype=np.float64).reshape(-1)
    st, par = [root], [-1]
    for i in range(1, n):
        cand = [j for j in range(max(0, i - 40), i) if j not in leaves]
        p = cand[rng.randint(len(cand))]
        for _ in range(64):
            s = move(space, rng, st[p], step)
            if near(space, s, root) <= reach:
                break
        else:
            s, p = move(space, rng, root, step), 0
        st.append(s)
        par.append(p)
    return np.array(st), np.array(par, dtype=np.int32)


def frame(S, name, scale, offset):
    """the R^n shape S moved whole: bounds, obstacles, trees and goals scaled, then translated.  A sphere that sits on a node of
    tree 0 (to the bit) sits on the moved node (to the bit)"""
    assert S["space"] == "rn"
    f = lambda x: np.asarray(x, dtype=np.float64) * scale + offset   # noqa: E731
    trees = [(f(s), p) for s, p in S["trees"]]
    sc = []
    for c in S["sph_c"]:
        on = [i for i, s in enumerate(S["trees"][0][0]) if np.array_equal(s, c)]
        sc.append(trees[0][0][on[0]] if on else f(c))
    return shape(name, "rn", S["dim"], trees, [(f(c), r * scale) for c, r in S["goals"]], (sc, S["sph_r"] * scale),
                 (f(S["box_lo"]), f(S["box_hi"])), bounds=[(float(f(lo)), float(f(hi))) for lo, hi in S["bounds"]],
                 fraction=S["fraction"], max_nodes=S["max_nodes"])


FAR_GOAL = 0.01   # the radius of a goal nobody is near


# ============================================================================================================ A: mixed sizes
A_SIZES = [1, 2, 64, 257, 1024, 65, 512, 1]
A_KILL = {1: [1], 3: [20, 200], 4: [100, 700, 1000], 5: [64]}       # problem -> nodes that get a small sphere; 2: nothing; 6: everything
A_SO3_SIZES = [1, 600, 130]
A_SO2_SIZES = [1, 300, 1024]


def a_root(p):
    return np.array([2.0 + 3.0 * (p % 3), 2.0 + 3.0 * (p // 3), 5.0])


@functools.lru_cache(maxsize=None)
def a_tree(p):
    return bushy("rn", A_SIZES[p], a_root(p), 7100 + p, 0.15, 0.5 if p == 6 else 1.3)


@functools.lru_cache(maxsize=None)
def mixed_rn():
    """one batch whose capacity the fifth tree fills.  Problem 6 lies whole inside one sphere (the root too: it is never tested)"""
    trees = [a_tree(p) for p in range(8)]
    sc, sr = [a_root(6)], [1.0]
    for p, nodes in sorted(A_KILL.items()):
        for i in nodes:
            sc.append(trees[p][0][i].copy())
            sr.append(rh.KILL_R)
    far = np.array([9.9, 9.9, 0.1])
    return shape("A_r3_mixed", "rn", 3, trees, [(far, FAR_GOAL)] * 8, (sc, sr), max_nodes=1024)


@functools.lru_cache(maxsize=None)
def mixed_257():
    """problem 3 of mixed_rn alone with its two spheres: the tree that family E moves into other frames"""
    st, par = a_tree(3)
    return shape("A_r3_257", "rn", 3, [(st, par)], [(np.array([9.9, 9.9, 0.1]), FAR_GOAL)],
                 ([st[i].copy() for i in A_KILL[3]], [rh.KILL_R] * 2))


def so3_stage_cap(P, cap, tiles):
    """oxhip_rrt_batch_revalidate_trees (oxhip_api.hip, `if (so3)`): the edges one staging chunk holds are
    max(64, min(P * cap * 6 / 65, P * tiles * 256)) -- 65 bytes a staged edge out of 6 bytes a slot"""
    return max(64, min(P * cap * 6 // 65, P * tiles * 256))


def so3_chunk_ends(S):
    """(problem, node slot) at which every staging chunk but the last ends: slot g of the flattened range is problem g / span, node
    g % span, span = tiles * 256 (reval_slot_edge, rrt_revalidate.hip)"""
    n = sizes(S)
    cap = (S["max_nodes"] + 1023) // 1024 * 1024
    tiles = (max(n) + 255) // 256
    span, stage = tiles * 256, so3_stage_cap(len(n), cap, tiles)
    return [(g // span, g % span) for g in range(stage, len(n) * span, stage)]


@functools.lru_cache(maxsize=None)
def mixed_so3():
    """P = 3, cap = 1024, tiles = 3: 3 * 1024 * 6 / 65 = 283 edges a chunk, span 768: the chunks end at slots 283, 566 (behind
    tree 0, before tree 1: between two problems), 849 = (1, 81) and 1132 = (1, 364) (inside tree 1), 1415 = (1, 647) (behind it) ..."""
    trees = [bushy("so3", n, rh.SO3_CENTRES[p], 7200 + p, 0.03, 0.35) for p, n in enumerate(A_SO3_SIZES)]
    kill = [(1, 50), (1, 80), (1, 81), (1, 364), (1, 599), (2, 10), (2, 129)]   # 80 / 81: the last slot of a chunk, the first of the next
    far = rh.quat_axis_half([0.0, 1.0, 0.0], 1.5)
    return shape("A_so3_mixed", "so3", 4, trees, [(far, 0.001)] * 3,
                 ([trees[p][0][i].copy() for p, i in kill], [rh.SO3_KILL_R] * len(kill)), max_nodes=1024)


def thin_arcs(centres, half=1e-5):
    return [[c - half] for c in centres], [[c + half] for c in centres]


@functools.lru_cache(maxsize=None)
def mixed_so2():
    trees = [bushy("so2", n, [c], 7300 + p, 0.02, 0.6) for p, (n, c) in enumerate(zip(A_SO2_SIZES, (-2.0, 0.0, 2.0)))]
    kill = [(1, 7), (1, 299), (2, 300), (2, 800), (2, 1023)]
    return shape("A_so2_mixed", "so2", 1, trees, [([3.0], 1e-6)] * 3, boxes=thin_arcs([float(trees[p][0][i][0]) for p, i in kill]),
                 max_nodes=1024)


# ============================================================================================================ B: moves
B_RANGES = {   # name -> (n, the old indices that must go)
    "tile_256": (1024, range(1, 257)), "tile_255": (1024, range(1, 256)), "tile_257": (1024, range(1, 258)),
    "every_second": (1024, range(1, 1024, 2)), "lone_survivor": (1025, range(1, 1024)), "only_node_1": (1024, [1]),
    "only_last": (1024, [1023]),
}


@functools.lru_cache(maxsize=None)
def move_tree(name):
    """R^2.  The nodes that go are a subtree under their lowest member, the head (a child of the root) and lie at x in 6 .. 9; all
    others hang under the root at x in 1 .. 4.  -> (states, parents, head)"""
    n, gone = B_RANGES[name]
    gone = list(gone)
    rng = np.random.RandomState(7400 + sorted(B_RANGES).index(name))
    st = np.column_stack([rng.uniform(1.0, 4.0, size=n), rng.uniform(1.0, 9.0, size=n)])
    par = np.full(n, -1, dtype=np.int32)
    kept_so_far, gone_so_far, going = [0], [], set(gone)
    for i in range(1, n):
        if i in going:
            st[i, 0] += 5.0
            par[i] = gone_so_far[-1 - rng.randint(min(3, len(gone_so_far)))] if gone_so_far else 0
            gone_so_far.append(i)
        else:
            par[i] = kept_so_far[-1 - rng.randint(min(3, len(kept_so_far)))]
            kept_so_far.append(i)
    return st, par, gone[0]


@functools.lru_cache(maxsize=None)
def moves():
    """all seven trees in one batch: one thin sphere on each head (no other tree has a tested state there, the model test asserts
    the removed sets)"""
    names = sorted(B_RANGES)
    trees = [move_tree(k) for k in names]
    return shape("B_moves", "rn", 2, [(s, p) for s, p, _ in trees], [([9.9, 0.1], FAR_GOAL)] * len(names),
                 ([s[h].copy() for s, _, h in trees], [THIN] * len(names)), max_nodes=1025, problems=names)


@functools.lru_cache(maxsize=None)
def move_256():
    """the first tree of B alone: the tree that family E moves into other frames"""
    s, p, h = move_tree("tile_256")
    return shape("B_tile_256", "rn", 2, [(s, p)], [([9.9, 0.1], FAR_GOAL)], ([s[h].copy()], [THIN]))


# ============================================================================================================ C: sphere windows
C_COUNTS = [63, 64, 65, 128, 129]
C_N = 130
C_EDGE = 97          # the edge that the decisive sphere cuts: node 97 and its parent


def c_legs():
    """(dim, spheres, index of the decisive sphere in the table, two boxes as well)"""
    out = []
    for dim in (3, 8):
        for m in C_COUNTS:
            places = sorted({0, m - 1} | {k for k in (63, 64) if k < m})
            out += [(dim, m, k, False) for k in places]
            out.append((dim, m, m - 1, True))
    return out


@functools.lru_cache(maxsize=None)
def window_scene(dim, n_spheres, place, with_boxes):
    """a wide tree (edges of several steps); sphere `place` of the table is thin and sits on a tested state inside edge C_EDGE; every
    other sphere (radius 0.04) lies 0.1 from a node that is more than 1.5 from both ends of that edge"""
    st, par = bushy("rn", C_N, [5.0] * dim, 7500 + dim, 0.8, 4.5)
    base = shape("C_probe_r%d" % dim, "rn", dim, [(st, par)], [([0.0] * dim, 0.0)])
    ref = Ref(base)
    a, b = st[par[C_EDGE]], st[C_EDGE]
    n = ref.steps(a, b)
    assert n >= 2, "edge %d is tested at `to` only" % C_EDGE
    decisive = ref.tested_state(a, b, n // 2, n)
    sites = [j for j in range(1, C_N) if min(orc.distance(st[j], a), orc.distance(st[j], b)) > 1.5]
    assert len(sites) >= 32
    rng = np.random.RandomState(7600 + dim)

    def beside(k, gap):
        u = rng.normal(size=dim)
        return st[sites[k % len(sites)]] + gap * u / math.sqrt(float(u @ u))

    sc = [beside(k, 0.1) for k in range(n_spheres - 1)]
    sr = [0.04] * (n_spheres - 1)
    sc.insert(place, decisive)
    sr.insert(place, THIN)
    boxes = None
    if with_boxes:   # both beside nodes far from the edge: the box loop runs after the windows of spheres
        c = [beside(5, 0.2), beside(17, 0.2)]
        boxes = ([v - 0.05 for v in c], [v + 0.05 for v in c])
    far = np.array([9.9] + [0.1] * (dim - 1))
    return shape("C_r%d_%d_at%d%s" % (dim, n_spheres, place, "_boxes" if with_boxes else ""), "rn", dim, [(st, par)], [(far, FAR_GOAL)],
                 (sc, sr), boxes, decisive=place)


# ============================================================================================================ D: steps, direction
D_FRACTION = 0.003        # res = 0.003 * sqrt(200) * 0.1 = 0.00424: 2,000 steps are 8.5 long and fit the bounds


def _steps_after(ref, x_exact, k):
    """the first x above x_exact (ulp by ulp) at which a motion of length x takes k + 1 steps, and how many ulps that took"""
    x, m = x_exact, 0
    while ref.steps([0.0, 0.0], [x, 0.0]) == k:
        x, m = float(np.nextafter(x, np.inf)), m + 1
        assert m <= 4
    return x, m


@functools.lru_cache(maxsize=None)
def steps_scene():
    """R^2, two problems.  Problem 0: under the root at (0, 0.25) one parent per case at (0, y) and its child at (length, y), so that
    the edge's distance is the child's x exactly.  `cases`: name -> (node, expected num_steps, expected verdict by construction); the
    verdicts asserted come from the oracle.  Problem 1: a root inside a sphere of radius 0.8 res, children at 0.9, 1.5 and 3.5 res."""
    probe = shape("D_probe", "rn", 2, [([[0.0, 0.0]], [-1])], [([0.0, 0.0], 0.0)], fraction=D_FRACTION)
    ref, res = Ref(probe), resolution(probe)
    st, par, cases, sc, sr = [[0.0, 0.25]], [-1], {}, [[0.0, 0.25]], [THIN]   # the root carries a thin sphere: nobody tests it ...
    st.append([0.0, 0.25])                                                    # ... but node 1, its copy, is tested at `to`
    par.append(0)
    cases["duplicate_of_root_in_obstacle"] = (1, 0, False)

    def case(name, y, length, n_steps, kept, sphere_x=None, r=None):
        i = len(st)
        st.extend([[0.0, y], [length, y]])
        par.extend([0, i])
        cases[name] = (i + 1, n_steps, kept)
        if sphere_x is not None:
            sc.append([sphere_x, y])
            sr.append(r)

    case("duplicate", 0.5, 0.0, 0, True)
    case("half_res", 1.0, 0.5 * res, 1, True, 0.25 * res, 0.05 * res)          # strictly between the two: never tested
    for k in (1, 2):
        exact = k * res
        above, ulps = _steps_after(ref, exact, k)
        assert ulps >= 1
        first = above / (k + 1)   # the first state that k + 1 steps test; k steps test length / k first
        for name, length, n_steps in (("k%d_exact" % k, exact, k), ("k%d_below" % k, float(np.nextafter(exact, 0.0)), k),
                                      ("k%d_above" % k, above, k + 1)):
            case(name, 1.0 + k + 0.25 * len(cases), length, n_steps, n_steps == k, first, 0.02 * res)
    case("long", 9.0, 1999.5 * res, 2000, False)
    i = cases["long"][0]
    sc.append(ref.tested_state(np.array(st[i - 1]), np.array(st[i]), 1990))   # ten steps before its far end
    sr.append(0.2 * res)
    root = np.array([5.0, 5.0])
    kids = [root + np.array([0.9 * res, 0.0]), root + np.array([0.0, 1.5 * res]), root - np.array([3.5 * res, 0.0])]
    sc.append(root)
    sr.append(0.8 * res)
    return shape("D_steps", "rn", 2, [(st, par), ([root] + kids, [-1, 0, 0, 0])], [([9.9, 0.1], FAR_GOAL)] * 2, (sc, sr),
                 fraction=D_FRACTION, cases=cases)


# ============================================================================================================ E: outside, frames
E_FRACTION = 1.0          # res = a tenth of the extent: the 1,000-long motions take about 700 steps (1e5-long ones would take 70,000)
E_DIMS = [2, 6]
FRAMES = [(1.0, 1e3), (1.0, 1e6), (1e-12, 0.0), (1e18, 0.0), (1e60, 0.0)]   # (scale, offset)


def rn_tested_states(a, b, n):
    """all n states that check_motion(a -> b) tests, [n][dim]: orc_interpolate's three roundings per coordinate, over whole arrays"""
    t = np.arange(1, n + 1, dtype=np.float64) / float(n)
    return a[None, :] + (b - a)[None, :] * t[:, None]


def rn_distances(c, states):
    """orc_distance(c, state) per row: the sequential sum from 0.0, then the square root"""
    acc = np.zeros(len(states))
    for k in range(states.shape[1]):
        d = c[k] - states[:, k]
        acc = acc + d * d
    return np.sqrt(acc)


@functools.lru_cache(maxsize=None)
def outside_scene(dim):
    """bounds [0, 10]^dim.  Problem 0 has its root inside them, problem 1 at x = 1e5 (setup does not test a start).  roles: name ->
    (problem, node, kind); kind `through`: a sphere of radius 0.8 on a tested state; `graze`: the radius is the smallest distance from
    the centre to a tested state (cut by one comparison); `miss`: that radius one ulp smaller (kept); `far`: nothing near"""
    pad = lambda *v: list(v) + [5.0] * (dim - len(v))   # noqa: E731
    t0 = ([pad(5.0, 5.0), pad(2.0, 8.0), pad(-50.0, 5.0), pad(1e3, 1e3), pad(-50.0, 1e3), pad(-60.0, 12.0), pad(-55.0, 14.0)],
          [-1, 0, 0, 1, 3, 0, 5])
    t1 = ([pad(1e5, 5.0), pad(1e5, 1e3), pad(1e5 + 20.0, 5.0), pad(1e5 - 30.0, 40.0), pad(1e5 + 7.0, -9.0), pad(1e5 - 31.0, 43.0)],
          [-1, 0, 0, 0, 3, 3])
    roles = dict(in_in_far=(0, 1, "far"), in_out_through=(0, 2, "through"), in_out_far=(0, 3, "far"), out_out_graze=(0, 4, "graze"),
                 in_out_miss=(0, 5, "miss"), out_out_short_far=(0, 6, "far"), e5_graze=(1, 1, "graze"), e5_through=(1, 2, "through"),
                 e5_miss=(1, 3, "miss"), e5_far=(1, 4, "far"), e5_short_far=(1, 5, "far"))
    base = shape("E_r%d" % dim, "rn", dim, [t0, t1], [(pad(9.9, 0.1), FAR_GOAL)] * 2, fraction=E_FRACTION)
    ref, sc, sr, sphere_of = Ref(base), [], [], {}
    for name, (p, i, kind) in roles.items():
        if kind == "far":
            continue
        st, par = base["trees"][p]
        a, b = st[par[i]], st[i]
        n = ref.steps(a, b)
        if kind == "through":
            c, r = ref.tested_state(a, b, n // 2, n), 0.8
        else:
            # beside a state inside the motion, pushed on along it and a little sideways
            u = (b - a) / orc.distance(a, b)
            side = np.zeros(dim)
            side[1 if abs(u[0]) > 0.5 else 0] = 0.05
            c = ref.tested_state(a, b, n // 2, n) + 0.4 * u + side
            r = float(rn_distances(c, rn_tested_states(a, b, n)).min())
            if kind == "miss":
                r = float(np.nextafter(r, 0.0))
        sphere_of[name] = len(sr)
        sc.append(c)
        sr.append(r)
    return shape(base["name"], "rn", dim, base["trees"], base["goals"], (sc, sr), fraction=E_FRACTION, roles=roles, sphere_of=sphere_of)


@functools.lru_cache(maxsize=None)
def framed(which, k):
    base = dict(a257=mixed_257, b256=move_256)[which]()
    scale, offset = FRAMES[k]
    return frame(base, "E_%s_x%g_plus%g" % (which, scale, offset), scale, offset)


# ============================================================================================================ F: goal
F_CENTRE, F_RADIUS = np.array([1.0, 1.0, 1.0]), 0.625      # 0.625 = 5 / 8: along (3, 4, 0) / 5 the offsets are 0.375 and 0.5, exact
F_ULPS = [-2, -1, 0, 1, 2]


def _ulps(x, k):
    for _ in range(abs(k)):
        x = float(np.nextafter(x, math.inf if k > 0 else -math.inf))
    return x


@functools.lru_cache(maxsize=None)
def threshold_scene():
    """one problem per probe, the tree a root and the probe: goal_node is 1 or -1.  Probes: distance == radius exactly and one and two
    ulps of the coordinate to either side, along the x axis and along the 3-4-5 diagonal"""
    probes = [("axis%+d" % k, [_ulps(1.625, k), 1.0, 1.0]) for k in F_ULPS] + [("diag%+d" % k, [_ulps(1.375, k), 1.5, 1.0]) for k in F_ULPS]
    trees = [([[5.0, 5.0, 5.0], s], [-1, 0]) for _, s in probes]
    return shape("F_threshold", "rn", 3, trees, [(F_CENTRE, F_RADIUS)] * len(probes), probes=[k for k, _ in probes])


F_N = 800
F_SAT = [3, 300, 700]
F_LANE = [3, 300, 515, 700]   # 3 and 515 = 3 + 2 * 256 are the same thread's, two tiles apart: its own `best` must be the minimum too
F_LEGS = {   # name -> (satisfying nodes, those of them killed); None: only the root satisfies
    "none": (F_SAT, []), "lowest": (F_SAT, [3]), "two_lowest": (F_SAT, [3, 300]), "all": (F_SAT, [3, 300, 700]),
    "same_thread": (F_LANE, []), "root_only": None}
F_WHERE = dict(   # space -> (problem roots, edge step, reach, goal offset from the root, goal radius, spread of the three, kill radius)
    rn=([a_root(p) for p in range(6)], 0.15, 1.0, 1.3, 0.05, 0.035, THIN),
    so3=([np.array(q) for q in ([0.0, 0.0, 0.0, 1.0], [1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.5, 0.5, 0.5, 0.5],
                               [0.5, 0.5, -0.5, 0.5])],
         0.03, 0.3, 0.4, 0.05, 0.03, rh.SO3_KILL_R),
    so2=([np.array([c]) for c in (-2.6, -1.6, -0.6, 0.4, 1.4, 2.4)], 0.02, 0.25, 0.4, 0.05, 0.03, 1e-5))


@functools.lru_cache(maxsize=None)
def ladder_scene(space):
    """six problems, each in a region of its own.  Nodes 3, 300 and 700 (one per tile, leaves) lie in the goal ball, which is
    outside the tree's reach; problem by problem none, the lowest, the two lowest, all three carry a thin obstacle; in the fifth
    node 515 satisfies as well.  In the sixth problem the goal ball is round the root and no obstacle is near"""
    roots, step, reach, off, radius, spread, kill_r = F_WHERE[space]
    trees, goals, kills = [], [], []
    for p, (leg, what) in enumerate(F_LEGS.items()):
        st, par = bushy(space, F_N, roots[p], 7700 + p, step, reach, leaves=F_LANE)
        st = st.copy()
        if what is None:
            goals.append((roots[p], 1e-6 if space == "so2" else 1e-3))
        else:
            nodes, killed = what
            if space == "so3":
                centre = rh.quat_mul(roots[p], rh.quat_axis_half([1.0, 0.3, 0.0], off))
                at = [rh.quat_mul(centre, rh.quat_axis_half(ax, spread)) for ax in ([1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 1.0, 0.0])]
            else:
                e0 = np.eye(len(roots[p]))[0]
                centre = roots[p] + off * e0
                at = [centre + spread * v for v in ((e0, -e0, 0.0 * e0, 0.5 * e0) if space == "so2" else (e0, -e0, np.roll(e0, 1), -np.roll(e0, 1)))]
            for i, s in zip(nodes, at):
                st[i] = s
            goals.append((centre, radius))
            kills += [st[i].copy() for i in killed]
        trees.append((st, par))
    sph, boxes = (kills, [kill_r] * len(kills)), None
    if space == "so2":
        sph, boxes = None, thin_arcs([float(c[0]) for c in kills], kill_r)
    return shape("F_ladder_%s" % space, space, 3, trees, goals, sph, boxes, legs=list(F_LEGS))


# ============================================================================================================ G: twins
G_N, G_BIG = 400, 1802
G_LEGS = {   # name -> (n, [groups of equal nodes, the first (odd: it dies with node 1) below the others (even)], the group at the goal)
    "pair_5_70": (G_N, [[5, 70]], 0), "pair_5_300": (G_N, [[5, 300]], 0), "pair_63_64": (G_N, [[63, 64]], 0),
    "pair_far_tiles": (G_BIG, [[401, 1800]], 0),                   # the lower twin would have been 201st, the upper becomes node 900
    "triple_5_70_300": (G_N, [[5, 70, 300]], 0),
    "signed_zero": (G_N, [[5, 70]], 0),
    "four_in_a_wave": (G_N, [[7, 130], [9, 140], [11, 150], [13, 160]], 3),   # 130 .. 160 become nodes 65 .. 80: one wave
}
G_CLEAR = 0.6     # no other node within this of a goal centre; the twins lie at 0.2


@functools.lru_cache(maxsize=None)
def twin_scene():
    """R^3, one problem per leg, the interleaved tree of rrt_revalidate_helpers (odd nodes under node 1, even under node 2) and one
    thin sphere on node 1: every odd node goes.  Groups of equal nodes, one of them 0.2 from the goal centre, the others further"""
    base, _ = rh.rn_tree(3, G_BIG, "interleave", (3.6, 6.4), 7800)
    trees, goals = [], []
    for name, (n, groups, at_goal) in G_LEGS.items():
        st = base[:n].copy()
        centre = np.array([5.0, 5.0, 0.2]) if name == "signed_zero" else np.array([5.0, 5.0, 5.0])
        crowd = np.sqrt(((st - centre) ** 2).sum(axis=1)) < G_CLEAR + 0.1
        st[crowd, 2] += 1.5
        for g, members in enumerate(groups):
            spot = centre - np.array([0.0, 0.0, 0.2]) if g == at_goal else np.array([4.0 + 0.1 * g, 8.5, 8.5])
            for i in members:
                st[i] = spot
        if name == "signed_zero":
            assert st[70, 2] == 0.0
            st[5, 2] = -0.0
        trees.append((st, rh.topology("interleave", n, None)))
        goals.append((centre, 0.05))
    return shape("G_twins", "rn", 3, trees, goals, ([base[1].copy()], [THIN]), max_nodes=2048, legs=list(G_LEGS))
