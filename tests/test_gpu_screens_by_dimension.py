"""GPU: the binary32 screens in every dimension they serve, in moved and scaled frames and at the underflow end.

Every planner names nearest / radius candidates with a binary32 screen and decides in binary64 under an error bound that
depends on D (screen_margins in rrt_device.hpp: stream kernel, RRT*, RRTConnect; E = u H^2 D (3D + 9) in rrt_lanes.hip and
rrt_cells.hip; the PRM radius and k-nearest screens).  These tests run those branches for D = 1 .. 8 -- RRT in frames moved
to 1e6 and scaled from 1e-158 (binary64 squares subnormal) through 1e-40 (binary32 coordinates subnormal) and 1e-20 (binary32
squares underflowing) to 1e100, planted near ties, the margin sweep with its far side taken from the error model, RRT* and
PRM in frames -- bit for bit against the CPU oracle.  tests/test_screen_error_model.py checks the bounds themselves."""
import functools
import math

import numpy as np
import pytest

from helpers import bits
from prm_helpers import make_oracle_prm

pytestmark = pytest.mark.gpu

from oxmpl_amd import capi, scenarios  # noqa: E402
from oracle import oracle_py as orc  # noqa: E402

KNAME = {capi.KERNEL_STREAM: "stream", capi.KERNEL_RESIDENT: "resident", capi.KERNEL_LANES: "lanes", capi.KERNEL_CELLS: "cells",
         capi.KERNEL_AUTO: "auto"}
SCREENED = (capi.KERNEL_LANES, capi.KERNEL_CELLS)   # kernels that count their exact-path events (stamps()[4])


def kernels_for(dim):
    """every kernel kind that serves R^dim: stream everywhere, lanes R^2 .. R^6, cells and resident R^2 / R^3, and AUTO"""
    ks = [capi.KERNEL_STREAM]
    if 2 <= dim <= 6:
        ks.append(capi.KERNEL_LANES)
    if dim in (2, 3):
        ks += [capi.KERNEL_CELLS, capi.KERNEL_RESIDENT]
    return ks + [capi.KERNEL_AUTO]


def _gpu_for(sc, n_problems, max_nodes, stop, seed, first_pid=0, kernel=0):
    try:
        return scenarios.make_batch(sc, n_problems, max_nodes, stop, seed, first_pid, 0, kernel)
    except capi.OxhipError as e:
        if e.status == capi.ERR_BAD_ARG and ("resident" in str(e) or "cell-grid kernel" in str(e)):
            pytest.skip("this kernel has no instantiation for this shape")
        raise


def _oracle_for(sc, seed, pid, max_nodes, stop):
    p = orc.OracleRRT(sc["dim"], sc["bounds"], sc["max_distance"], sc["goal_bias"], sc["lvs_fraction"], max_nodes, stop, seed, pid)
    if sc["spheres"] is not None:
        p.set_spheres(*sc["spheres"])
    if sc["boxes"] is not None:
        p.set_boxes(*sc["boxes"])
    p.setup(sc["start"], sc["goal_centre"], sc["goal_radius"])
    return p


def _assert_same_problem(gpu, p, o, c=None):
    c = c or gpu.counts()
    assert int(c["nodes"][p]) == o.num_nodes
    assert int(c["iterations"][p]) == o.iterations
    assert int(c["accepted"][p]) == o.accepted
    assert int(c["checksum"][p]) == o.checksum
    assert int(c["goal_node"][p]) == o.goal_node
    gs, gp = gpu.tree(p)
    os_, op = o.tree()
    assert np.array_equal(gp, op)
    assert np.array_equal(bits(gs), bits(os_))
    assert np.array_equal(bits(gpu.path(p)), bits(o.path()))


def frame(sc, scale, offset):
    """the scene with every coordinate mapped to x scale + offset, every length scaled"""
    t = lambda v: np.asarray(v, dtype=np.float64) * scale + offset
    out = dict(sc, bounds=[(float(t(lo)), float(t(hi))) for lo, hi in sc["bounds"]], max_distance=sc["max_distance"] * scale,
               start=list(t(sc["start"])), goal_centre=list(t(sc["goal_centre"])), goal_radius=sc["goal_radius"] * scale)
    if sc["spheres"] is not None:
        out["spheres"] = (t(sc["spheres"][0]), np.asarray(sc["spheres"][1], dtype=np.float64) * scale)
    if sc["boxes"] is not None:
        out["boxes"] = (t(sc["boxes"][0]), t(sc["boxes"][1]))
    return out


def dim_scene(dim, goal_bias=0.1):
    """a seeded scene per dimension, built like test_rrt_other_dimensions_and_obstacle_mixes's: spheres plus one box"""
    rng = np.random.default_rng(900 + dim)
    ns = {1: 2, 2: 6, 3: 12, 4: 16, 5: 20, 6: 24, 7: 24, 8: 24}[dim]
    lo = rng.random((1, dim)) * 6.0 - 1.0
    return dict(dim=dim, bounds=[(-3.0, 7.0)] * dim, max_distance=0.7, goal_bias=goal_bias, lvs_fraction=0.02,
                start=[-2.5] * dim, goal_centre=[6.5] * dim, goal_radius=0.4,
                spheres=(rng.random((ns, dim)) * 6.0 - 1.0, rng.random(ns) * 0.5 + 0.1),
                boxes=(lo, lo + rng.random((1, dim)) * 0.8 + 0.1))


# ------------------------------------------------------------------------------------- 1. RRT frame sweep, every dim
# offsets: binary32 separates little (1e6: nothing); 1e-12 .. 1e-158: binary32 squares underflow (1e-20), binary32 coordinates
# are subnormal (1e-40), binary64 squares are subnormal (1e-158); 1e18: binary32 squares untrusted, 1e30 / 1e100: overflow
# (1e-23: binary32 products land in the subnormal range, where a rounding errs by 2^-150 whatever the value -- the term E lacked)
FRAMES = [(1.0, 1.0e3), (1.0, 1.0e6), (1.0, -5.0e4), (1.0e-12, 0.0), (1.0e-20, 0.0), (1.0e-23, 0.0), (1.0e-40, 0.0),
          (1.0e-158, 0.0), (1.0e18, 0.0), (1.0e30, 0.0), (1.0e100, 0.0)]
P_FRAME, ITERS_FRAME, NODES_FRAME = 4, 700, 600


@functools.lru_cache(maxsize=None)
def _frame_oracles(dim, scale, offset):
    sc = frame(dim_scene(dim), scale, offset)
    planners = [_oracle_for(sc, 31, 40 + p, NODES_FRAME, False) for p in range(P_FRAME)]
    orc.solve_many(planners, ITERS_FRAME, threads=P_FRAME)
    return sc, planners


@pytest.mark.parametrize("scale,offset", FRAMES, ids=["%g%+g" % f for f in FRAMES])
@pytest.mark.parametrize("dim,kernel", [(d, k) for d in range(1, 9) for k in kernels_for(d)],
                         ids=["r%d-%s" % (d, KNAME[k]) for d in range(1, 9) for k in kernels_for(d)])
def test_rrt_frames_in_every_dimension(dim, kernel, scale, offset):
    sc, planners = _frame_oracles(dim, scale, offset)
    gpu = _gpu_for(sc, P_FRAME, NODES_FRAME, False, 31, 40, kernel)
    gpu.solve(ITERS_FRAME)
    c = gpu.counts()
    for p in range(P_FRAME):
        _assert_same_problem(gpu, p, planners[p], c)
    assert min(o.num_nodes for o in planners) > 100   # the scene still lets the trees grow
    gpu.close()


# ------------------------------------------------------------------------------------- 2. near ties, every dim
N_PLANT = 3000


def lanes_locate(i, S, C):
    """rrt_lanes.hip Layout4<S, C>::locate: (scanner thread, register row) of node i"""
    common = C * 512
    if i < common:
        return (i & 2047) >> 2, (i >> 11) * 4 + (i & 3)
    r = i - common
    blk, c = r // 1536, r % 1536
    ht = c >> 2
    return [3, 2, 7, 6, 1, 5][ht >> 6] * 64 + (ht & 63), C + blk * 4 + (c & 3)


def lanes_rows(dim, cap):
    """pick_rows_lanes<D> (rrt_lanes.hip): (S, C) of the instantiation that serves a tree of capacity cap"""
    if cap <= 2048:
        return 4, 4
    return (24, 16) if dim in (2, 3) else (20, 20)


def tie_pairs(dim, cap):
    """index pairs that land, in the lane kernel's shape for this D, in one lane (other register row), in neighbouring lanes,
    in different waves and in different register-row blocks; both orders"""
    S, C = lanes_rows(dim, cap)
    want = {"same_lane": (5, 6), "next_lane": (5, 9), "other_wave": (5, 261), "other_block": (5, 2053),
            "far": (2999, 17), "wave_edge": (511, 512), "block_edge": (2047, 2048), "mixed": (1030, 70)}
    got = {}
    for name, (ia, ib) in want.items():
        (ta, ra), (tb, rb) = lanes_locate(ia, S, C), lanes_locate(ib, S, C)
        got[name] = (ta == tb, abs(ta - tb) == 1, ta >> 6 != tb >> 6, ra // 4 != rb // 4)
    assert got["same_lane"][0] and got["next_lane"][1] and got["other_wave"][2] and got["other_block"][3] and got["other_block"][0]
    assert got["wave_edge"][2] and got["block_edge"][3]
    pairs = list(want.values())
    return pairs + [(b, a) for a, b in pairs]


def _d2(a, q):
    acc = None
    for x, y in zip(a, q):
        d = x - y
        acc = d * d if acc is None else acc + d * d
    return acc


def near_tie_pair(q, rng, scale):
    """test_gpu_parity._near_tie_pair at any scale: two states whose d2 to q differ but whose square roots coincide.  Where d2
    is a binary64 subnormal (scale 1e-158) sqrt is one-to-one and no such pair exists: there the pair is two distinct states
    whose d2 are equal (the exact tie: the lower index wins as well).  Far from the origin (offset 1e6) one ulp of a coordinate
    moves d2 by ~1e-10, a million ulps of d2: there the pair comes from a lattice of nudges of up to three coordinates, whose
    d2 values, sorted, hold neighbours one or two ulps apart."""
    subnormal = 0.81 * scale * scale < 2.2250738585072014e-308
    if max(abs(v) for v in q) * 2.0 ** -52 > 1e-12 * scale:
        dim = len(q)
        ks = list(range(dim - min(dim, 3), dim))
        reach = 150 if len(ks) == 2 else 20
        for _ in range(50):
            v = rng.standard_normal(dim)
            a = np.array([float(x + 0.9 * scale * w / np.linalg.norm(v)) for x, w in zip(q, v)])
            steps = np.stack(np.meshgrid(*[np.arange(-reach, reach + 1)] * len(ks), indexing="ij"), -1).reshape(-1, len(ks))
            cand = np.repeat(a[None, :], len(steps), axis=0)
            for j, k in enumerate(ks):
                ulp = np.spacing(np.abs(a[k]))
                cand[:, k] = a[k] + steps[:, j] * ulp   # (exact: a few ulps of a[k], inside its binade)
            d2 = (cand[:, 0] - q[0]) * (cand[:, 0] - q[0])
            for k in range(1, dim):
                d2 = d2 + (cand[:, k] - q[k]) * (cand[:, k] - q[k])
            order = np.argsort(d2, kind="stable")
            sd = d2[order]
            hit = np.nonzero((sd[1:] != sd[:-1]) & (np.sqrt(sd[1:]) == np.sqrt(sd[:-1])))[0]
            if len(hit):
                ia, ib = order[hit[0]], order[hit[0] + 1]
                pa, pb = [float(x) for x in cand[ia]], [float(x) for x in cand[ib]]
                da, db = _d2(pa, q), _d2(pb, q)
                assert da != db and math.sqrt(da) == math.sqrt(db)
                return pa, pb, da, db
        # R^2: the lattice of two nudged coordinates is too regular to put two d2 values an ulp apart; the exact tie instead,
        # q mirrored in its last coordinate (distinct states, equal d2)
        for _ in range(1000):
            v = rng.standard_normal(dim)
            a = [float(x + 0.9 * scale * w / np.linalg.norm(v)) for x, w in zip(q, v)]
            b = list(a)
            b[-1] = float(2.0 * q[-1] - a[-1])
            da, db = _d2(a, q), _d2(b, q)
            if b != a and da == db:
                return a, b, da, db
        raise AssertionError("no near-tie pair found")
    for _ in range(200000):
        v = rng.standard_normal(len(q))
        a = [float(x + 0.9 * scale * w / np.linalg.norm(v)) for x, w in zip(q, v)]
        da = _d2(a, q)
        b = list(a)
        for _k in range(40):
            b[-1] = float(np.nextafter(b[-1], np.inf))
            db = _d2(b, q)
            if (db == da and b != a) if subnormal else (db != da and math.sqrt(db) == math.sqrt(da)):
                return a, b, da, db
    raise AssertionError("no near-tie pair found")


def tie_scene(dim):
    start, goal = [0.5] * dim, [9.5] * dim
    sph = scenarios.sphere_field(seed=0x5EED0100 + dim, n=24, dim=dim, rmin=0.3, rmax=0.8 if dim <= 3 else 1.5,
                                 keep_clear=[start, goal])
    return dict(dim=dim, bounds=[(0.0, 10.0)] * dim, max_distance=0.5, goal_bias=0.0, lvs_fraction=0.05, start=start,
                goal_centre=goal, goal_radius=0.5, spheres=sph, boxes=None)


TIE_DIMS = [2, 4, 5, 6, 7, 8]
TIE_FRAMES = [(1.0, 0.0), (1.0, 1.0e6), (1.0e-158, 0.0)]


@pytest.mark.parametrize("scale,offset", TIE_FRAMES, ids=["%g%+g" % f for f in TIE_FRAMES])
@pytest.mark.parametrize("dim,kernel", [(d, k) for d in TIE_DIMS for k in kernels_for(d)],
                         ids=["r%d-%s" % (d, KNAME[k]) for d in TIE_DIMS for k in kernels_for(d)])
def test_near_ties_in_every_dimension(dim, kernel, scale, offset):
    """test_planner_near_ties_take_the_exact_path in R^dim: the strict '<' on the post-sqrt value keeps the lower index even
    when its d2 is the larger one, wherever the two nodes sit in the kernel's layout"""
    sc = frame(tie_scene(dim), scale, offset)
    cap = 4096
    cases = tie_pairs(dim, cap)
    P, n = len(cases), N_PLANT
    gpu = _gpu_for(sc, P, cap, False, 77, 0, kernel)
    rng = np.random.default_rng(123 + dim)
    planners, flipped, exact = [], 0, 0
    for p, (ia, ib) in enumerate(cases):
        r = orc.Rng(77, p)
        assert not r.random_bool(0.0)
        q = [r.random_range(lo, hi) for lo, hi in sc["bounds"]]
        a, b, da, db = near_tie_pair(q, rng, scale)
        far = rng.standard_normal((n, dim))   # every other node at least 3 (scaled) away from q
        far = np.array(q) + far / np.linalg.norm(far, axis=1, keepdims=True) * (3.0 + rng.random((n, 1)) * 4.0) * scale
        tree = far.copy()
        tree[ia], tree[ib] = a, b
        parents = np.concatenate([[-1], rng.integers(0, np.arange(1, n))]).astype(np.int32)
        o = _oracle_for(sc, 77, p, cap, False)
        assert o.set_tree(tree, parents) == 0
        gpu.set_tree(p, tree, parents)
        planners.append(o)
        d_lo, d_hi = (da, db) if ia < ib else (db, da)
        flipped += d_lo > d_hi   # a d2-argmin would pick the other node
        exact += da == db
        assert orc.nearest(tree, q)[0] == min(ia, ib)
    assert flipped + exact >= 3   # (exact ties: where d2 is subnormal, and in R^2 far from the origin)
    gpu.solve(1, freeze=True)
    c = gpu.counts()
    for p, o in enumerate(planners):
        o.solve(1, freeze=True)
        assert int(c["checksum"][p]) == o.checksum, cases[p]
        assert int(c["nodes"][p]) == n
    gpu.solve(300)   # the warm-started trees keep growing identically
    for p, o in enumerate(planners):
        o.solve(300)
        _assert_same_problem(gpu, p, o)
    gpu.close()


# ------------------------------------------------------------------------------ 3. margin sweep, every dim, model thresholds
MARGIN_EPS = [0.0, 2.0 ** -40, 2.0 ** -30, 2.0 ** -26, 2.0 ** -24, 2.0 ** -23, 2.0 ** -22, 2.0 ** -21, 2.0 ** -20, 2.0 ** -19,
              2.0 ** -18, 2.0 ** -17, 2.0 ** -16, 2.0 ** -15, 2.0 ** -14, 2.0 ** -12, 2.0 ** -10, 2.0 ** -8, 2.0 ** -7, 2.0 ** -6,
              2.0 ** -5, 2.0 ** -4]
D_MIN, H_SWEEP = 0.4, 5.0   # the planted nearest node's smallest distance; the largest |coordinate - c0| ([0, 10]^D, c0 = 5)


def far_side_eps(dim):
    """the relative gap beyond which the screen must decide, from the error model the lane and cell kernels document: nodes at d
    and d (1 + eps) differ by ~2 eps d^2 in d2, the scanners separate beyond 2.5E, E = u H^2 D (3D + 9); four times that"""
    e = 2.0 ** -24 * H_SWEEP ** 2 * dim * (3 * dim + 9)
    return 4.0 * 2.5 * e / (2.0 * D_MIN ** 2)


SWEEP_DIMS = [2, 4, 5, 6, 7, 8]


@pytest.mark.parametrize("dim,kernel", [(d, k) for d in SWEEP_DIMS for k in kernels_for(d)],
                         ids=["r%d-%s" % (d, KNAME[k]) for d in SWEEP_DIMS for k in kernels_for(d)])
def test_screen_margin_sweep_in_every_dimension(dim, kernel):
    """test_screen_margin_sweep in R^dim: the nearest node A at d, a runner-up B at d (1 + eps), both planted at index pairs of
    the kernel's layout for this D; results equal the oracle's whatever the screen decides, and the kernels that count exact-path
    events refuse to decide at eps <= 2^-22 and always decide at four times the error model's margin and beyond"""
    sc = tie_scene(dim)
    sc["goal_bias"] = 1.0
    q = np.array(sc["goal_centre"])
    pairs = tie_pairs(dim, 4096)
    n = N_PLANT
    rng = np.random.default_rng(2024 + dim)
    far_eps = far_side_eps(dim)
    assert any(e >= far_eps for e in MARGIN_EPS)
    amb_by_eps = {}
    for eps in MARGIN_EPS:
        P = len(pairs)
        gpu = _gpu_for(sc, P, 4096, False, 5, 0, kernel)
        planners = []
        for p, (ia, ib) in enumerate(pairs):
            u = rng.standard_normal((2, dim))
            u /= np.linalg.norm(u, axis=1, keepdims=True)
            d = D_MIN + 0.5 * rng.random()
            a = q - np.abs(u[0]) * d                      # inside the bounds: the goal centre sits near the upper corner
            b = q - np.abs(u[1]) * d * (1.0 + eps)
            far = rng.standard_normal((n, dim))
            far = q - np.abs(far / np.linalg.norm(far, axis=1, keepdims=True)) * (3.0 + rng.random((n, 1)) * 4.0)
            tree = far.copy()
            tree[ia], tree[ib] = a, b
            parents = np.concatenate([[-1], rng.integers(0, np.arange(1, n))]).astype(np.int32)
            o = _oracle_for(sc, 5, p, 4096, False)
            assert o.set_tree(tree, parents) == 0
            gpu.set_tree(p, tree, parents)
            planners.append(o)
        if kernel in SCREENED:
            gpu.enable_stamps(True)
        gpu.solve(8, freeze=True)
        c = gpu.counts()
        for p, o in enumerate(planners):
            o.solve(8, freeze=True)
            assert int(c["checksum"][p]) == o.checksum, (eps, pairs[p])
            assert int(c["iterations"][p]) == o.iterations == 8
        if kernel in SCREENED:
            amb_by_eps[eps] = int(gpu.stamps()[4])
            gpu.enable_stamps(False)
        gpu.solve(40)
        for p, o in enumerate(planners):
            o.solve(40)
            _assert_same_problem(gpu, p, o)
        gpu.close()
    if kernel in SCREENED:
        print("R^%d %s: exact-path events by eps %s (far side from %.3g)" % (dim, KNAME[kernel], amb_by_eps, far_eps))
        for eps, n_amb in amb_by_eps.items():
            if eps <= 2.0 ** -22:
                assert n_amb > 0, ("the screen decided a pair it cannot separate", eps, amb_by_eps)
            if eps >= far_eps:
                assert n_amb == 0, ("the screen does not decide beyond its documented margin", eps, far_eps, amb_by_eps)


# ------------------------------------------------------------------------------------------------ 4. RRT* in frames
STAR_DESIGNS = {"decoupled": capi.KERNEL_CELLS, "decoupled_lanes": capi.KERNEL_LANES, "one_kernel": capi.KERNEL_STREAM}
STAR_CASES = [(2, "decoupled"), (2, "decoupled_lanes"), (2, "one_kernel"),
              (5, "decoupled_lanes"), (5, "one_kernel")]   # (the cell-grid geometry serves R^2 / R^3 only)
STAR_FRAMES = [(1.0, 1.0e6), (1.0e-40, 0.0), (1.0e-158, 0.0), (1.0e30, 0.0)]


@pytest.mark.parametrize("scale,offset", STAR_FRAMES, ids=["%g%+g" % f for f in STAR_FRAMES])
@pytest.mark.parametrize("dim,design", STAR_CASES, ids=["r%d-%s" % c for c in STAR_CASES])
def test_rrt_star_frames_by_dimension(dim, design, scale, offset):
    sc = frame(dim_scene(dim), scale, offset)
    radius = 1.2 * scale
    n_prob, cap, iters = 4, 2000, 600
    g = capi.RRTBatch(dim, sc["bounds"], sc["max_distance"], sc["goal_bias"], n_prob, cap, sc["lvs_fraction"], False, 9, 300, 0,
                      STAR_DESIGNS[design], capi.PLANNER_RRT_STAR, radius)
    g.set_spheres(*sc["spheres"])
    g.set_boxes(*sc["boxes"])
    g.setup(sc["start"], sc["goal_centre"], sc["goal_radius"])
    g.solve(iters)
    cts = g.counts()
    for p in range(n_prob):
        o = orc.OracleRRTStar(dim, sc["bounds"], sc["max_distance"], sc["goal_bias"], radius, sc["lvs_fraction"], cap, False, 9,
                              300 + p)
        o.set_spheres(*sc["spheres"])
        o.set_boxes(*sc["boxes"])
        o.setup(sc["start"], sc["goal_centre"], sc["goal_radius"])
        o.solve(iters)
        assert o.num_nodes > 100
        assert int(cts["nodes"][p]) == o.num_nodes and int(cts["iterations"][p]) == o.iterations
        assert int(cts["accepted"][p]) == o.accepted and int(cts["checksum"][p]) == o.checksum
        assert int(cts["goal_node"][p]) == o.goal_node
        gs, gp = g.tree(p)
        os_, op = o.tree()
        assert np.array_equal(bits(gs), bits(os_)) and np.array_equal(gp, op)
        assert np.array_equal(bits(g.costs(p)), bits(o.costs()))
        gpath, opath = g.path(p), o.path()
        assert gpath.shape == opath.shape and np.array_equal(bits(gpath), bits(opath))
    g.close()


# ------------------------------------------------------------------------------------------------ 4. PRM in frames
def _prm_params(dim, scale, offset, radius, knn_k=0, n=1500):
    rng = np.random.default_rng(5 + dim)
    ns = 12 if dim <= 3 else 8
    centres = rng.uniform(1.0, 9.0, size=(ns, dim)) * scale + offset
    radii = rng.uniform(0.3, 0.9, size=ns) * (1.0 if dim <= 3 else 2.0) * scale
    lo, hi = 0.0 * scale + offset, 10.0 * scale + offset
    return dict(dim=dim, bounds=[(lo, hi)] * dim, radius=radius * scale, fraction=0.05, seed=123, stream=9, max_milestones=n,
                max_samples=10 ** 9, boxes=[], knn_k=knn_k, spheres=[(list(map(float, c)), float(r)) for c, r in zip(centres, radii)])


def _prm_run(P, scale, offset):
    from helpers import params_spheres
    dim = P["dim"]
    g = capi.PRMRoadmap(dim, P["bounds"], P["radius"], P["max_milestones"], 0.0, P["fraction"], 0, P["seed"], P["stream"], 0,
                        P["knn_k"])
    g.set_spheres(*params_spheres(P))
    o = make_oracle_prm(P)
    s, gc = [0.4 * scale + offset] * dim, [9.6 * scale + offset] * dim
    g.setup(s, gc, 1.0 * scale)
    o.setup(s, gc, 1.0 * scale)
    g.construct_roadmap()
    o.construct_roadmap(P["max_milestones"])
    n, e, smp = g.sizes()
    assert n == o.num_milestones and smp == o.num_samples
    gs, goff, gn = g.roadmap()
    os_, ooff, on = o.roadmap()
    assert np.array_equal(bits(gs), bits(os_))
    assert np.array_equal(goff, ooff) and np.array_equal(gn, on)
    st, path = g.solve(0.0)
    assert st == o.solve()
    opath = o.path()
    assert path.shape == opath.shape and np.array_equal(bits(path), bits(opath))
    return g, gn


PRM_FRAMES = [(1.0, 1.0e3), (1.0, 1.0e6), (1.0e-12, 0.0), (1.0e18, 0.0), (1.0e60, 0.0), (1.0e-40, 0.0), (1.0e-158, 0.0)]


@pytest.mark.parametrize("scale,offset", PRM_FRAMES, ids=["%g%+g" % f for f in PRM_FRAMES])
@pytest.mark.parametrize("dim", [2, 6])
def test_prm_radius_frames_by_dimension(dim, scale, offset):
    g, gn = _prm_run(_prm_params(dim, scale, offset, 0.6 if dim == 2 else 3.5), scale, offset)
    assert len(gn) > 1500     # a connected-ish roadmap, not a degenerate one
    g.close()


KNN_SCALES = [1.0e-40, 1.0e-158, 1.0e60, 1.0e-60]


@pytest.mark.parametrize("scale", KNN_SCALES, ids=["%g" % s for s in KNN_SCALES])
@pytest.mark.parametrize("dim", [3, 6])
def test_prm_knn_frames_by_dimension(dim, scale):
    """k = 8 nearest: in R^6 at 1e60 the host's density volume (oxhip_prm_api.hip) overflows to inf, at 1e-60 it underflows to
    0; the roadmap must still be the oracle's"""
    g, gn = _prm_run(_prm_params(dim, scale, 0.0, 1.3 if dim == 3 else 3.5, knn_k=8), scale, 0.0)
    print("k-NN PRM R^%d at scale %g: exact rows %d" % (dim, scale, g.knn_exact_rows()))
    assert len(gn) > 1500
    g.close()
