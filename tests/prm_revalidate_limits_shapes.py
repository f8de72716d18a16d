"""Shapes for planting a roadmap (oxhip_prm_set_roadmap) and re-checking it (oxhip_prm_revalidate, prm_revalidate.hip, DESIGN.md
section 20) at the limits the constructed scenes of tests/test_gpu_prm_revalidate.py do not reach:
  A  space      every space (R^1 .. R^8, SO(3)): 300 milestones, about six neighbours a row, spheres only / boxes only / both
  B  windows    R^3, 63 / 64 / 65 / 128 / 129 spheres, the decisive one the last of the table (the midpoint filter's windows of 64)
  C  steps      duplicate milestones, half a resolution, dist / res at, just below and just above 1 and 2, a 2,000-step edge
  D  outside    milestones at -50, 1e3 and 1e5 with bounds [0, 10]^d: edges cut, grazed (cut by one comparison, kept by one ulp), far
  E  csr        empty rows in front, inside and behind, 254 .. 514 entries, K_24, hubs of 300 -- in R^3 and in SO(3) --
                with the first / the last / the one-but-last entry's edge cut, everything cut, nothing cut
  F  reuse      roadmaps of 1,200, 40 and 1,300 milestones and two nested scenes, for one handle
  G  refusals   a roadmap of 1,024 milestones (16 blocks of entries) broken rule by rule, and `first_violation`, the rule checker

A shape is a dict: name, so3, dim (4 on SO(3)), bounds, fraction, states [n][dim], lists (edge lists), sph_c / sph_r (SO(3):
cones), box_lo / box_hi.  Plain numpy and Python: nothing here loads the GPU library.  The verdicts are the references': the C
oracle (oracle/rrt_oracle.c through oracle_py.OracleRRT) over R^n, tests/golden/make_golden_so3.py (Cones, check_motion) over
SO(3) -- `Ref` and `cpu_filter` below.  Thin obstacles sit on a state that the reference's check_motion tests (`tested_state`),
with radius 1e-9: they cut that edge whatever the geometry around it.  Shapes and verdicts are computed once (functools caches)
and shared: never modify one.  tests/test_prm_revalidate_limits_model.py holds every shape to the property it exists for."""
import functools
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden as mg  # noqa: E402
import make_golden_so3 as g3  # noqa: E402

from oracle import oracle_py as orc  # noqa: E402
from prm_revalidate_helpers import csr, plain_filter, symmetric_lists  # noqa: E402

FRACTION = 0.05
SO3_BOUNDS = [0.0, 0.0, 0.0, 1.0, math.pi]      # the whole of SO(3)
THIN = 1e-9


def rn_bounds(dim):
    return [(0.0, 10.0)] * dim


def shape(name, dim, states, lists, sph=None, boxes=None, so3=False, fraction=FRACTION, **extra):
    w = 4 if so3 else dim
    sc, sr = sph if sph is not None else ([], [])
    bl, bh = boxes if boxes is not None else ([], [])
    S = dict(name=name, so3=so3, dim=w, bounds=SO3_BOUNDS if so3 else rn_bounds(dim), fraction=fraction,
             states=np.array(states, dtype=np.float64).reshape(-1, w), lists=[list(r) for r in lists],
             sph_c=np.array(sc, dtype=np.float64).reshape(-1, w), sph_r=np.array(sr, dtype=np.float64).reshape(-1),
             box_lo=np.array(bl, dtype=np.float64).reshape(-1, w), box_hi=np.array(bh, dtype=np.float64).reshape(-1, w))
    assert len(S["states"]) == len(S["lists"]) and len(S["sph_c"]) == len(S["sph_r"]) and len(S["box_lo"]) == len(S["box_hi"])
    for a in ("states", "sph_c", "sph_r", "box_lo", "box_hi"):
        S[a].setflags(write=False)
    S.update(extra)
    return S


def with_obstacles(S, name, sph=None, boxes=None, **more):
    """the shape S among other obstacles"""
    extra = {k: v for k, v in S.items() if k not in ("name", "so3", "dim", "bounds", "fraction", "states", "lists", "sph_c", "sph_r",
                                                     "box_lo", "box_hi")}
    extra.update(more)
    return shape(name, S["dim"], S["states"], S["lists"], sph if sph is not None else (S["sph_c"], S["sph_r"]),
                 boxes if boxes is not None else (S["box_lo"], S["box_hi"]), so3=S["so3"], fraction=S["fraction"], **extra)


# ============================================================================================================ the references
def resolution(S):
    """what check_motion divides the distance by: a tenth of the longest valid segment"""
    return (g3.lvsl(S["fraction"]) if S["so3"] else orc.maximum_extent(S["bounds"]) * S["fraction"]) * 0.1


def distance(S, a, b):
    return g3.distance(list(map(float, a)), list(map(float, b))) if S["so3"] else orc.distance(a, b)


def steps(S, a, b):
    """check_motion's num_steps for the motion a -> b"""
    if S["so3"]:
        return mg.num_steps(distance(S, a, b), g3.lvsl(S["fraction"]))
    return orc.num_steps(orc.distance(a, b), orc.maximum_extent(S["bounds"]) * S["fraction"])


def tested_state(S, a, b, k, n=None):
    """the k-th state that check_motion(a -> b) tests, k = 1 .. num_steps (to the bit: the reference's own interpolate)"""
    n = steps(S, a, b) if n is None else n
    assert 1 <= k <= n
    t = float(k) / float(n)
    if S["so3"]:
        return np.array(g3.interpolate(list(map(float, a)), list(map(float, b)), t))
    return orc.interpolate(a, b, t)


def edges_of(lists):
    """the undirected edges as (j, i), j > i: the motions the re-check tests, from j to i, in CSR order of their lower entries"""
    return [(j, i) for j, row in enumerate(lists) for i in row if i < j]


class Ref:
    """is_valid / check_motion of the shape's space among its obstacles (or a part of them), by the reference implementations"""

    def __init__(self, S, spheres=True, boxes=True, n_spheres=None):
        c, r = (S["sph_c"], S["sph_r"]) if spheres else (S["sph_c"][:0], S["sph_r"][:0])
        if n_spheres is not None:
            c, r = c[:n_spheres], r[:n_spheres]
        self.S = S
        if S["so3"]:
            self.cones = g3.Cones([([float(v) for v in cc], float(rr)) for cc, rr in zip(c, r)])
        else:
            d = S["dim"]
            self.o = orc.OracleRRT(d, S["bounds"], 1.0, 0.05, S["fraction"])
            if len(r):
                self.o.set_spheres(c, r)
            if boxes and len(S["box_lo"]):
                self.o.set_boxes(S["box_lo"], S["box_hi"])
            self.o.setup([0.0] * d, [0.0] * d, 0.0)

    def is_valid(self, s):
        return self.cones.is_valid([float(v) for v in s]) if self.S["so3"] else self.o.is_valid(s)

    def check_motion(self, a, b):
        if self.S["so3"]:
            return g3.check_motion(self.cones, self.S["fraction"], [float(v) for v in a], [float(v) for v in b])
        return self.o.check_motion(a, b)


_FILTERS = {}


def cpu_filter(S, lists=None, key=None, **part):
    """the plain filter by the references: dict(valid, ok {(j, i): verdict, between valid ends only}, kept, invalid, cut, kept_edges).
    `lists`: another roadmap over the same states (with a `key` that names it); `part`: Ref's choice of obstacles"""
    k = (S["name"], key, tuple(sorted(part.items())))
    assert (lists is None) == (key is None)
    if k not in _FILTERS:
        ref, st = Ref(S, **part), S["states"]
        ll = S["lists"] if lists is None else lists
        valid = np.array([ref.is_valid(s) for s in st], dtype=bool).reshape(-1)
        ok = {(j, i): ref.check_motion(st[j], st[i]) for j, i in edges_of(ll) if valid[i] and valid[j]}
        kept = plain_filter(ll, valid, ok)
        _FILTERS[k] = dict(valid=valid, ok=ok, kept=kept, invalid=int(np.count_nonzero(~valid)),
                           cut=sum(1 for v in ok.values() if not v), kept_edges=sum(len(r) for r in kept) // 2)
    return _FILTERS[k]


def counts(S, f=None):
    f = cpu_filter(S) if f is None else f
    return "%-28s n %4d entries %5d spheres %3d boxes %2d | invalid %3d  cut between valid ends %4d  kept %4d" % (
        S["name"], len(S["lists"]), sum(len(r) for r in S["lists"]), len(S["sph_r"]), len(S["box_lo"]), f["invalid"], f["cut"],
        f["kept_edges"])


# ============================================================================================================ points and graphs
def points(so3, dim, n, seed):
    rng = np.random.default_rng(seed)
    if so3:
        q = rng.normal(size=(n, 4))
        return q / np.sqrt((q * q).sum(axis=1))[:, None]
    return rng.uniform(0.5, 9.5, size=(n, dim))


def near_graph(states, so3, k=3):
    """every milestone joined to the k nearest of the earlier ones (about 2k neighbours a row): a geometric graph; which pairs it
    takes is the shape's business, no verdict depends on it"""
    pairs = []
    for j in range(1, len(states)):
        if so3:
            d = np.arccos(np.minimum(np.abs(states[:j] @ states[j]), 1.0))
        else:
            d = np.sqrt(((states[:j] - states[j]) ** 2).sum(axis=1))
        pairs += [(j, int(i)) for i in np.argsort(d, kind="stable")[:k]]
    return symmetric_lists(len(states), pairs)


def ring_lists(n, nodes):
    """a ring through `nodes` (ascending global indices) in a roadmap of n milestones; every other row is empty"""
    m = len(nodes)
    return symmetric_lists(n, [(nodes[k], nodes[(k + 1) % m]) for k in range(m)])


def on_edge(S, j, i, k=None):
    """a state that check_motion(j -> i) tests, strictly inside the edge (num_steps // 2 unless told)"""
    a, b = S["states"][j], S["states"][i]
    n = steps(S, a, b)
    assert n >= 2, "edge (%d, %d) of %s is tested at `to` only" % (j, i, S["name"])
    return tested_state(S, a, b, n // 2 if k is None else k, n)


# ============================================================================================================ A: every space
DIMS = list(range(1, 9))
A_N = 300
A_LEGS = [(d, leg) for d in DIMS for leg in ("spheres", "boxes", "both")] + [(0, "cones")]


@functools.lru_cache(maxsize=None)
def space_scene(dim, leg):
    """dim = 0: SO(3).  Three edges get a sphere (cone) on a tested state and three others a box there; one milestone lies in a
    sphere and another in a box.  Obstacle radius: a tenth of the edge, so both ends stay clear of it"""
    so3 = dim == 0
    st = points(so3, dim, A_N, 20261020 + dim)
    base = shape("A_%s_%s" % ("so3" if so3 else "r%d" % dim, leg), dim, st, near_graph(st, so3), so3=so3, fraction=0.25 if so3 else FRACTION)
    long_edges = [e for e in edges_of(base["lists"]) if steps(base, st[e[0]], st[e[1]]) >= 4]
    assert len(long_edges) >= 12
    pick = [long_edges[len(long_edges) * q // 7] for q in range(1, 7)]
    sc, sr, bl, bh = [], [], [], []
    if leg != "boxes":
        for j, i in pick[:3]:
            sc.append(on_edge(base, j, i))
            sr.append(min(0.1 * distance(base, st[j], st[i]), 0.3))
        sc.append(st[A_N // 2].copy())
        sr.append(0.02)
    if leg in ("boxes", "both"):
        for j, i in pick[3:]:
            c, h = on_edge(base, j, i), min(0.1 * distance(base, st[j], st[i]), 0.3) / math.sqrt(dim)
            bl.append(c - h)
            bh.append(c + h)
        bl.append(st[A_N // 3] - 0.02)
        bh.append(st[A_N // 3] + 0.02)
    return with_obstacles(base, base["name"], (sc, sr), (bl, bh))


# ============================================================================================================ B: sphere windows
B_COUNTS = [63, 64, 65, 128, 129]
B_LEGS = [(m, False) for m in B_COUNTS] + [(129, True)]


@functools.lru_cache(maxsize=None)
def window_scene(n_spheres, with_boxes):
    """four planted edges near x = 2; spheres 1 .. m - 2 far away at x >= 6 (the filter drops them), sphere 0 beside edge (3, 2) without
    touching it (it stays in that motion's mask), the LAST sphere on a tested state of edge (1, 0)"""
    st = [[1.0 + 2.0 * (k % 2), 1.0 + 2.0 * (k // 2), 1.0 + 0.5 * (k % 2)] for k in range(8)]
    lists = symmetric_lists(8, [(1, 0), (3, 2), (5, 4), (7, 6)])
    base = shape("B_%d%s" % (n_spheres, "_boxes" if with_boxes else ""), 3, st, lists)
    far = [[6.0 + 0.25 * (k % 12), 1.0 + 0.25 * ((k // 12) % 12), 8.0] for k in range(n_spheres - 2)]
    beside = on_edge(base, 3, 2) + np.array([0.0, 0.0, 0.3])
    sc = [beside] + far + [on_edge(base, 1, 0)]
    sr = [0.1] + [0.1] * len(far) + [0.05]
    boxes = None
    if with_boxes:   # one box far away, one round a tested state of edge (5, 4): the box loop runs after two windows of spheres
        c = on_edge(base, 5, 4)
        boxes = ([[8.0, 8.0, 1.0], list(c - 0.05)], [[8.5, 8.5, 1.5], list(c + 0.05)])
    return with_obstacles(base, base["name"], (sc, sr), boxes)


# ============================================================================================================ C: step counts
C_FRACTION = 0.003        # res = 0.003 * sqrt(200) * 0.1 = 0.00424: 2,000 steps are 8.5 long and fit the bounds


def _steps_after(S, x_exact, k):
    """the first x above x_exact (ulp by ulp) at which a motion of length x takes k + 1 steps, and how many ulps that took"""
    x, m = x_exact, 0
    while steps(S, [0.0, 0.0], [x, 0.0]) == k:
        x, m = float(np.nextafter(x, np.inf)), m + 1
        assert m <= 4
    return x, m


@functools.lru_cache(maxsize=None)
def steps_scene():
    """R^2, every pair on a horizontal line of its own, from x = 0 (so that the pair's distance is its `to`'s x, exactly).  `pairs`:
    name -> (j, i, expected num_steps, expected verdict by construction); the verdicts asserted come from the oracle"""
    probe = shape("C_probe", 2, [[0.0, 0.0]], [[]], fraction=C_FRACTION)
    res = resolution(probe)
    st, pairs, sc, sr, edges = [], {}, [], [], []

    def pair(name, y, length, n_steps, kept, sphere_x=None, r=None):
        i = len(st)
        st.extend([[0.0, y], [length, y]])      # index i (`to` of the motion) at x = 0, index i + 1 (`from`) at x = length
        edges.append((i + 1, i))
        pairs[name] = (i + 1, i, n_steps, kept)
        if sphere_x is not None:
            sc.append([sphere_x, y])
            sr.append(r)

    pair("duplicate", 0.5, 0.0, 0, True)
    pair("half_res", 1.0, 0.5 * res, 1, True, 0.25 * res, 0.05 * res)          # strictly between the two: never tested
    for k in (1, 2):
        exact = k * res
        above, ulps = _steps_after(probe, exact, k)
        assert ulps >= 1
        # k + 1 steps test from + length / (k + 1) first: only the `above` motion has a state there (k steps: the first is at length / k)
        at = lambda length: length - length / (k + 1)   # noqa: E731  (seen from `to`, which lies at x = 0)
        for name, length, n_steps in (("k%d_exact" % k, exact, k), ("k%d_below" % k, float(np.nextafter(exact, 0.0)), k),
                                      ("k%d_above" % k, above, k + 1)):
            pair(name, 1.0 + k + 0.25 * len(pairs), length, n_steps, n_steps == k, at(above), 0.02 * res)
    pair("long", 9.0, 1999.5 * res, 2000, False)
    base = shape("C_steps", 2, st, symmetric_lists(len(st), edges), fraction=C_FRACTION)
    j, i = pairs["long"][:2]
    sc.append(tested_state(base, base["states"][j], base["states"][i], 1990))   # ten steps before its far end
    sr.append(0.2 * res)
    return with_obstacles(base, "C_steps", (sc, sr), pairs=pairs)


# ============================================================================================================ D: outside the bounds
D_FRACTION = 1.0          # res = a tenth of the extent: the 1e5-long motions take about 1e5 steps
D_DIMS = [2, 6]


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
    """roles: name -> (j, i, kind); kind `through`: a sphere of radius 0.8 on a tested state; `graze`: the radius is the smallest
    distance from the centre to a tested state (cut by one comparison); `miss`: that radius one ulp smaller (kept); `far`: nothing near"""
    pad = lambda *v: list(v) + [5.0] * (dim - len(v))   # noqa: E731
    st = [pad(5.0, 5.0), pad(2.0, 8.0), pad(-50.0, 5.0), pad(1e3, 1e3), pad(1e5, 5.0), [1e5] * dim, pad(-50.0, 1e3), pad(5.0, 1e5)]
    roles = dict(out_in_through=(2, 0, "through"), out_in_far=(3, 1, "far"), out_in_graze=(4, 0, "graze"), out_in_miss=(4, 1, "miss"),
                 out_out_far=(5, 3, "far"), out_out_through=(6, 2, "through"), out_out_graze=(7, 5, "graze"), out_in_miss2=(7, 0, "miss"))
    base = shape("D_r%d" % dim, dim, st, symmetric_lists(len(st), [(j, i) for j, i, _ in roles.values()]), fraction=D_FRACTION)
    S, sc, sr, sphere_of = base["states"], [], [], {}
    for name, (j, i, kind) in roles.items():
        if kind == "far":
            continue
        n = steps(base, S[j], S[i])
        inward = name.startswith("out_in")
        if kind == "through":
            c, r = tested_state(base, S[j], S[i], n - 5 if inward else n // 2, n), 0.8
        else:
            # beside the last state before `to` (the state farthest from the midpoint that is not an end), pushed on along the motion
            # and a little sideways: as near the rim of the filter's ball as a sphere that decides a motion between valid ends gets
            u = (S[i] - S[j]) / orc.distance(S[j], S[i])
            side = np.zeros(dim)
            side[1 if abs(u[0]) > 0.5 else 0] = 0.05
            c = tested_state(base, S[j], S[i], n - 1 if inward else n // 2, n) + 0.4 * u + side
            r = float(rn_distances(c, rn_tested_states(S[j], S[i], n)).min())
            if kind == "miss":
                r = float(np.nextafter(r, 0.0))
        sphere_of[name] = len(sr)
        sc.append(c)
        sr.append(r)
    return with_obstacles(base, base["name"], (sc, sr), roles=roles, sphere_of=sphere_of)


def filter_slack(S, j, i, sphere):
    """motion_valid_seq's midpoint filter (motion_seq.hpp) restated for the motion j -> i and one sphere, with the margin the re-check
    passes (SeqSpace::motion_margin over the handle's filt_abs = 1e-9 * max(1, |bounds|, |centres|)): the sphere is dropped when
    d(centre, mid) > sqrt((r + h)^2 (1 + 1e-9)), h = dist / 2 * (1 + 1e-6) + filt.  Returns (slack = that limit - d(centre, mid),
    margin = what h and the limit add to r + dist / 2)"""
    a, b, c, r = S["states"][j], S["states"][i], S["sph_c"][sphere], float(S["sph_r"][sphere])
    filt = 1e-9 * max(1.0, max(abs(v) for bb in S["bounds"] for v in bb), float(np.abs(S["sph_c"]).max()))
    filt = max(filt, 1e-9 * float(np.maximum(np.abs(a), np.abs(b)).max()))
    dist = orc.distance(a, b)
    mid = orc.interpolate(a, b, 0.5)
    h = 0.5 * dist * (1.0 + 1e-6) + filt
    limit = math.sqrt((r + h) * (r + h) * (1.0 + 1e-9))
    return limit - orc.distance(c, mid), limit - (r + 0.5 * dist)


# ============================================================================================================ E: CSR shapes
E_KINDS = ["front_empty", "inner_runs", "tail_empty", "entries_254", "entries_256", "entries_258", "entries_512", "entries_514", "k24",
           "hub_first", "hub_last"]
E_PLACEMENTS = ["first", "last", "pred", "all", "none"]
E_SO3_FRACTION = 1.0      # res = 0.157: a handful of steps per edge, so that the Python checker stays quick


def csr_lists(kind):
    if kind == "front_empty":                    # 300 empty rows, then a ring of 65
        return ring_lists(365, list(range(300, 365)))
    if kind == "inner_runs":                     # a ring of 65 with runs of 2 and of 70 empty rows inside it
        return ring_lists(137, list(range(0, 20)) + list(range(22, 40)) + list(range(110, 137)))
    if kind == "tail_empty":                     # a ring of 65, then 600 empty rows: n + 1 > n_entries, blocks that hold offsets only
        return ring_lists(665, list(range(65)))
    if kind.startswith("entries_"):              # a ring: two entries a milestone (a symmetric CSR holds an even number of entries)
        m = int(kind.split("_")[1]) // 2
        return ring_lists(m, list(range(m)))
    if kind == "k24":
        return [[v for v in range(24) if v != u] for u in range(24)]
    if kind == "hub_first":
        return [list(range(1, 301))] + [[0]] * 300
    assert kind == "hub_last"
    return [[300]] * 300 + [list(range(300))]


@functools.lru_cache(maxsize=None)
def csr_base(kind, so3):
    lists = csr_lists(kind)
    for attempt in range(50):   # random points, drawn again until every edge has a tested state strictly inside it (two steps or more)
        st = points(so3, 3, len(lists), 7000 + E_KINDS.index(kind) + (100 if so3 else 0) + 1000 * attempt)
        S = shape("E_%s_%s" % ("so3" if so3 else "r3", kind), 3, st, lists, so3=so3, fraction=E_SO3_FRACTION if so3 else FRACTION)
        if all(steps(S, st[j], st[i]) >= 2 for j, i in edges_of(lists)):
            return S
    raise AssertionError("no point set for " + kind)


def entry_edge(lists, e):
    """the undirected edge (j, i), j > i, that CSR entry e belongs to"""
    for u, row in enumerate(lists):
        if e < len(row):
            return max(u, row[e]), min(u, row[e])
        e -= len(row)
    raise IndexError(e)


@functools.lru_cache(maxsize=None)
def csr_scene(kind, so3, placement):
    """thin obstacles (radius 1e-9) on a tested state of: the first entry's edge / the last entry's / the one-but-last entry's /
    every edge; `none`: one thin obstacle that lies on no tested state"""
    base = csr_base(kind, so3)
    n_entries = sum(len(r) for r in base["lists"])
    if placement == "none":
        c = [np.array(g3.normalise([0.3, -0.2, 0.5, 0.1]))] if so3 else [np.array([9.9, 9.9, 9.9])]
    else:
        cut = dict(first=[entry_edge(base["lists"], 0)], last=[entry_edge(base["lists"], n_entries - 1)],
                   pred=[entry_edge(base["lists"], n_entries - 2)], all=edges_of(base["lists"]))[placement]
        c = [on_edge(base, j, i) for j, i in cut]
    return with_obstacles(base, base["name"] + "_" + placement, (c, [THIN] * len(c)))


# ============================================================================================================ F: one handle, reused
F_SIZES = [1200, 40, 1300]


@functools.lru_cache(maxsize=None)
def reuse_scene(so3, n, level):
    """level 1: scene S1 (two edges cut, one milestone covered); level 2: S2, S1's obstacles and three more; level 0: no obstacle"""
    st = points(so3, 3, n, 9000 + n + (1 if so3 else 0))
    base = shape("F_%s_%d_s%d" % ("so3" if so3 else "r3", n, level), 3, st, near_graph(st, so3), so3=so3,
                 fraction=E_SO3_FRACTION if so3 else FRACTION)
    long_edges = [e for e in edges_of(base["lists"]) if steps(base, st[e[0]], st[e[1]]) >= 2]
    assert len(long_edges) >= 8
    pick = [long_edges[len(long_edges) * q // 6] for q in range(1, 6)]
    c = [on_edge(base, *pick[0]), on_edge(base, *pick[1]), st[n // 2].copy(), on_edge(base, *pick[2]), on_edge(base, *pick[3]), st[n // 3].copy()]
    r = [0.02, THIN, 0.01, 0.02, THIN, 0.01]
    m = {0: 0, 1: 3, 2: 6}[level]
    return with_obstacles(base, base["name"], (c[:m], r[:m]))


# ============================================================================================================ G: refusals
G_N = 1024
RULES = ["offsets_start", "offsets_order", "neighbour_range", "self_loop", "unsorted", "asymmetric"]   # section 20's order


def first_violation(n, offsets, nbrs):
    """(rule, lowest offending row) of the first broken rule in section 20's order, None for a roadmap that is accepted"""
    off = [int(v) for v in offsets]
    if off[0] != 0:
        return "offsets_start", 0
    if any(off[i + 1] < off[i] for i in range(n)):
        return "offsets_order", min(i for i in range(n) if off[i + 1] < off[i])
    rows = [[int(v) for v in nbrs[off[u]:off[u + 1]]] for u in range(n)]
    checks = [("neighbour_range", lambda u, k, v: v >= n), ("self_loop", lambda u, k, v: v == u),
              ("unsorted", lambda u, k, v: k > 0 and rows[u][k - 1] >= v), ("asymmetric", lambda u, k, v: u not in rows[v])]
    for rule, broken in checks:   # (the later rules are asked only of a roadmap that passed the earlier ones)
        bad = [u for u in range(n) for k, v in enumerate(rows[u]) if broken(u, k, v)]
        if bad:
            return rule, min(bad)
    return None


@functools.lru_cache(maxsize=None)
def refusal_base():
    """1,024 milestones in R^3, each joined to its ring neighbours and to the milestones 37 away: 4,096 entries, 16 blocks; row 255
    ends block 3 and row 256 begins block 4"""
    st = points(False, 3, G_N, 4242)
    lists = symmetric_lists(G_N, [(u, (u + d) % G_N) for u in range(G_N) for d in (1, 37)])
    assert all(len(r) == 4 for r in lists)
    return shape("G_base", 3, st, lists)


def row_entry_block(lists, u):
    """the 256-entry block (one workgroup of the entry kernels) in which row u begins"""
    return sum(len(r) for r in lists[:u]) // 256


def break_rule(lists, rule, u, w=None):
    """breaks `rule` in row u of the edge lists (in place).  The later rules may break with it: the checker says which is reported"""
    row = lists[u]
    if rule == "neighbour_range":
        row[-1] = len(lists)                     # the row's last entry; it stays ascending
    elif rule == "self_loop":
        lists[u] = sorted(set(row[1:]) | {u})    # still strictly ascending
    elif rule == "unsorted":
        row[-2], row[-1] = row[-1], row[-2]      # found at the row's last entry
    else:
        assert rule == "asymmetric"
        w = row[1] if w is None else w
        lists[w].remove(u)                       # u's entry for w has lost its mirror: the offending row is u


REFUSALS = {   # name -> [(rule, row), ...] broken together
    **{"%s_255_256" % r: [(r, 255), (r, 256)] for r in RULES[2:]},
    **{"%s_0_last" % r: [(r, G_N - 1), (r, 0)] for r in RULES[2:]},
    **{"%s_256_last" % r: [(r, G_N - 1), (r, 256)] for r in RULES[2:]},
    **{"%s_last" % r: [(r, G_N - 1)] for r in RULES[2:]},         # range and unsorted: the offending entry is the roadmap's very last
    "offsets_start": [("offsets_start", 0)],
    "offsets_order_255_256": [("offsets_order", 255), ("offsets_order", 256)],
    "offsets_order_0_last": [("offsets_order", G_N - 1), ("offsets_order", 0)],    # (offsets[0] > offsets[1] breaks offsets_start first)
    "offsets_order_256_last": [("offsets_order", G_N - 1), ("offsets_order", 256)],
    "offsets_order_last": [("offsets_order", G_N - 1)],
    "offsets_start_and_order": [("offsets_start", 0), ("offsets_order", 700)],
    "all_entry_rules": [("asymmetric", 10), ("unsorted", 300), ("self_loop", 600), ("neighbour_range", 900)],
    "unsorted_then_lower_rows_asymmetric": [("unsorted", 800), ("asymmetric", 5)],
    "self_loop_then_lower_rows_unsorted": [("self_loop", 1000), ("unsorted", 2)],
    "unsorted_row_hides_asymmetry": [("unsorted", 513), ("asymmetric", 512, 513)],   # row 512 has lost its mirror in row 513, the unsorted one
}


@functools.lru_cache(maxsize=None)
def refusal(name):
    """(offsets u64, neighbours u32, (rule, row) the checker expects) of the base roadmap broken as REFUSALS[name] says.  Offsets are
    broken so that offsets[n] stays the length of the neighbour array: the call reads that many neighbours"""
    lists = [list(r) for r in refusal_base()["lists"]]
    breaks = REFUSALS[name]
    for rule, u, *w in breaks:
        if not rule.startswith("offsets"):
            break_rule(lists, rule, u, *w)
    off, nb = csr(lists)
    off = off.copy()
    for rule, u, *_ in sorted(breaks, key=lambda b: -b[1]):   # (from the highest row down: each leaves the rows below it as they were)
        if rule == "offsets_start":
            off[0] = 1
        elif rule == "offsets_order":            # offsets[u] rises above offsets[u + 1]; below u nothing decreases
            off[u] = int(off[u + 1]) + 1
    assert int(off[-1]) == len(nb)
    want = first_violation(G_N, off, nb)
    assert want is not None
    off.setflags(write=False)
    nb.setflags(write=False)
    return off, nb, want


@functools.lru_cache(maxsize=None)
def accepted_edge_cases():
    """name -> shape: roadmaps that must be accepted"""
    st = points(False, 3, G_N, 4243)
    return dict(
        empty_first_and_last_rows=shape("G_empty_ends", 3, st, ring_lists(G_N, list(range(1, G_N - 1)))),
        no_entries=shape("G_no_entries", 3, st[:300], [[] for _ in range(300)], ([st[7].copy()], [0.01])))
