"""GPU parity tests of BASELINE.json configs[3]: RRTConnect over the build-defined SE(2) space among line
segments (rrt_connect_se2.hip) through the C ABI, against the CPU oracle (oracle/se2_oracle.c) and the golden
fixtures (tests/golden/se2_golden.json).  Bit-exact: both trees, checksums, merged paths, and the SO(2) / SE(2)
arithmetic itself (fmod-based normalisation on the device).
PARITY UNPINNED against oxmpl: the reference has no SE(2) space (docs/BACKLOG.md:12-14)."""
import json
import math
import os

import numpy as np
import pytest

from helpers import unhex, bits

pytestmark = pytest.mark.gpu

from oxmpl_amd import capi, scenarios  # noqa: E402
from oracle import oracle_py as orc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def se2_golden():
    with open(os.path.join(ROOT, "tests", "golden", "se2_golden.json")) as f:
        return json.load(f)


def segs_of(P):
    return np.array([[unhex(v) for v in s] for s in P["segments"]], dtype=np.float64).reshape(-1, 4)


def make_oracle(P, seed, pid, max_nodes=None):
    o = orc.OracleSE2Connect(P["bounds_xy"], P["theta_bounds"], P["max_distance"], P["goal_bias"], P["fraction"],
                             max_nodes or P["max_nodes"], seed, pid)
    o.set_segments(segs_of(P), P["clearance"])
    o.setup(P["start"], P["goal"], P["goal_r"])
    return o


def make_gpu(P, n_problems, seed, first_pid, max_nodes=None, debug_flags=0):
    bounds = list(P["bounds_xy"]) + [tuple(P["theta_bounds"])]
    g = capi.RRTBatch(3, bounds, P["max_distance"], P["goal_bias"], n_problems, max_nodes or P["max_nodes"], P["fraction"],
                      True, seed, first_pid, 0, capi.KERNEL_AUTO, capi.PLANNER_RRT_CONNECT, 0.0, capi.SPACE_SE2,
                      debug_flags=debug_flags)
    g.set_segments(segs_of(P), P["clearance"])
    g.setup(P["start"], P["goal"], P["goal_r"])
    return g


def assert_same(g, p, o, c=None, gc=None):
    c = c or g.counts()
    gc = gc or g.goal_counts()
    assert int(c["nodes"][p]) == o.num_nodes(0) and int(gc["nodes"][p]) == o.num_nodes(1)
    assert int(c["iterations"][p]) == o.iterations and int(c["checksum"][p]) == o.checksum
    assert int(c["goal_node"][p]) == o.end_node(0) and int(gc["end_node"][p]) == o.end_node(1)
    for w, (gs, gp) in enumerate((g.tree(p), g.goal_tree(p))):
        os_, op = o.tree(w)
        assert np.array_equal(bits(gs), bits(os_)) and np.array_equal(gp, op)
    gpath, opath = g.path(p), o.path()
    assert gpath.shape == opath.shape and np.array_equal(bits(gpath), bits(opath))


def test_so2_se2_arithmetic_on_the_device(se2_golden):
    """normalise / distance / interpolate bit for bit, incl. the wrap-around edges and large angles (fmod)"""
    rng = np.random.default_rng(7)
    n = 20000
    a = np.column_stack([rng.uniform(-10, 10, n), rng.uniform(-10, 10, n), rng.uniform(-7, 7, n)])
    b = np.column_stack([rng.uniform(-10, 10, n), rng.uniform(-10, 10, n), rng.uniform(-7, 7, n)])
    # edges: +-PI, values one ulp around them, huge and tiny angles
    pi = math.pi
    edge = np.array([pi, -pi, np.nextafter(pi, 0), np.nextafter(-pi, 0), np.nextafter(pi, 4), 3 * pi, -5 * pi, 1e6, -1e9,
                     1e-300, -0.0, 0.0, 2 * pi, -2 * pi, 1e15])
    m = len(edge)
    a[:m * m, 2] = np.repeat(edge, m)
    b[:m * m, 2] = np.tile(edge, m)
    t = rng.uniform(0, 1, n)
    t[:64] = np.linspace(0.0, 1.0, 64)
    out0 = capi.se2_op_batch(0, a, b)
    out1 = capi.se2_op_batch(1, a, b, t)
    L = orc.lib()
    for i in list(range(m * m)) + list(range(m * m, n, 37)):
        assert out0[i, 0] == orc.se2_distance(a[i], b[i]) or (math.isnan(out0[i, 0]))
        assert bits(out0[i, 1:2])[0] == bits(np.array([L.orc_so2_normalise(a[i, 2])]))[0]
        assert bits(out0[i, 2:3])[0] == bits(np.array([L.orc_so2_distance(a[i, 2], b[i, 2])]))[0]
        assert np.array_equal(bits(out1[i]), bits(orc.se2_interpolate(a[i], b[i], float(t[i]))))
    # the reference's own exact unit-test vector (so2_state.rs:80-87): normalise(3 PI / 2) == -PI / 2
    assert capi.se2_op_batch(0, [[0.0, 0.0, 3.0 * math.pi / 2.0]], [[0.0, 0.0, 0.0]])[0, 1] == -math.pi / 2.0
    for k in se2_golden["kat"]["random"]:
        x, y = [unhex(v) for v in k["a"]], [unhex(v) for v in k["b"]]
        o0 = capi.se2_op_batch(0, [x], [y])[0]
        assert [("%016x" % int(v)) for v in bits(o0)] == [k["se2_distance"], k["so2_normalise"], k["so2_distance"]]
        o1 = capi.se2_op_batch(1, [x], [y], [unhex(k["t"])])[0]
        assert [("%016x" % int(v)) for v in bits(o1)] == k["se2_interpolate"]


@pytest.mark.parametrize("key", ["soup256", "gap"])
def test_se2_connect_golden_scenes(se2_golden, key):
    P = se2_golden[key]["params"]
    for r in se2_golden[key]["runs"]:
        g = make_gpu(P, 1, r["seed"], r["pid"])
        st = g.solve(P["max_iterations"])
        assert st[0] == capi.OK
        c, gc = g.counts(), g.goal_counts()
        assert [int(c["nodes"][0]), int(gc["nodes"][0])] == r["n"] and int(c["iterations"][0]) == r["iterations"]
        assert "%016x" % int(c["checksum"][0]) == r["checksum"]
        assert [int(c["goal_node"][0]), int(gc["end_node"][0])] == r["end"]
        want = np.array([[unhex(v) for v in row] for row in r["path"]]).reshape(-1, 3)
        got = g.path(0)
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
        o = make_oracle(P, r["seed"], r["pid"])
        o.solve(P["max_iterations"])
        assert_same(g, 0, o, c, gc)
        # the checker and the motion check, batched, on the path
        assert g.is_valid(got).all() and g.check_motion(got[:-1], got[1:]).all()
        g.close()


def test_se2_connect_batch_and_checker_parity(se2_golden):
    """64 problems of the 256-segment scene in one launch; is_valid / check_motion against the oracle on random states"""
    P = se2_golden["soup256"]["params"]
    g = make_gpu(P, 64, 11, 500)
    st = g.solve(10 ** 6)
    assert (st == capi.OK).all()
    c, gc = g.counts(), g.goal_counts()
    for p in range(0, 64, 7):
        o = make_oracle(P, 11, 500 + p)
        assert o.solve(10 ** 6) == orc.SOLVED
        assert_same(g, p, o, c, gc)
    rng = np.random.default_rng(3)
    n = 4000
    a = np.column_stack([rng.uniform(0, 10, n), rng.uniform(0, 10, n), rng.uniform(-math.pi, math.pi, n)])
    b = a + np.column_stack([rng.normal(0, 0.4, n), rng.normal(0, 0.4, n), rng.normal(0, 1.5, n)])
    o = make_oracle(P, 0, 0)
    v = g.is_valid(a)
    m = g.check_motion(a, b)
    assert 0.2 < v.mean() < 0.98                        # the scene is neither empty nor full
    for i in range(0, n, 3):
        assert bool(v[i]) == o.is_valid(a[i])
        assert bool(m[i]) == o.check_motion(a[i], b[i])


def test_se2_node_cap_and_argument_validation(se2_golden):
    P = dict(se2_golden["gap"]["params"])
    # goal unreachable: enclosed by four segments -> both trees fill up to the node cap
    box = [(8.0, 4.0, 10.0, 4.0), (8.0, 6.0, 10.0, 6.0), (8.0, 4.0, 8.0, 6.0), (10.0, 4.0, 10.0, 6.0)]
    P["segments"] = [["%016x" % int(bits(np.array([v]))[0]) for v in s] for s in box]
    g = make_gpu(P, 2, 1, 0, max_nodes=300)
    st = g.solve(10 ** 6)
    c, gc = g.counts(), g.goal_counts()
    assert (st == capi.ERR_NO_SOLUTION_FOUND).all() and (c["stop_reason"] == capi.STOP_NODES).all()
    for p in range(2):
        o = make_oracle(P, 1, p, max_nodes=300)
        assert o.solve(10 ** 6) == orc.NO_SOLUTION_FOUND
        assert_same(g, p, o, c, gc)
    for kw, status in ((dict(dim=2, bounds=[(0.0, 1.0)] * 2), capi.ERR_BAD_ARG),                       # (x, y, theta) needs dim 3
                       (dict(bounds=[(0.0, 1.0), (0.0, 1.0), (1.0, 1.0)]), capi.ERR_ZERO_VOLUME),       # so2_state_space.rs:59-64
                       (dict(planner=capi.PLANNER_RRT), capi.ERR_BAD_ARG)):
        args = dict(dim=3, bounds=[(0.0, 1.0), (0.0, 1.0), (-1.0, 1.0)], max_distance=0.5, goal_bias=0.05, n_problems=1,
                    planner=capi.PLANNER_RRT_CONNECT, space=capi.SPACE_SE2)
        args.update(kw)
        with pytest.raises(capi.OxhipError) as ei:
            capi.RRTBatch(**args)
        assert ei.value.status == status


def hexsegs(segs):
    return [["%016x" % int(bits(np.array([float(v)]))[0]) for v in s] for s in segs]


def test_se2_without_the_segment_grid_and_in_chunks(se2_golden):
    """The grid lookup of the motion check switched off (every state against every segment), and a solve cut into launches of 37
    iterations (the block sampler starts over inside its 64-iteration blocks): same trees, checksums and paths"""
    P = se2_golden["soup256"]["params"]
    ref = make_gpu(P, 12, 21, 40)
    assert (ref.solve(10 ** 6) == capi.OK).all()
    c0, gc0 = ref.counts(), ref.goal_counts()
    plain = make_gpu(P, 12, 21, 40, debug_flags=capi.DEBUG_SE2_NO_SEGMENT_GRID)
    assert (plain.solve(10 ** 6) == capi.OK).all()
    small = make_gpu(P, 12, 21, 40, debug_flags=capi.DEBUG_SE2_SMALL_LDS)   # the shape of batches larger than the chip
    assert (small.solve(10 ** 6) == capi.OK).all()
    chunked = make_gpu(P, 12, 21, 40)
    for _ in range(4000):
        st = chunked.solve(37)
        if (st == capi.OK).all():
            break
    assert (st == capi.OK).all()
    for g in (plain, small, chunked):
        c, gc = g.counts(), g.goal_counts()
        for k in ("nodes", "iterations", "checksum", "goal_node"):
            assert np.array_equal(c[k], c0[k]), k
        assert np.array_equal(gc["nodes"], gc0["nodes"]) and np.array_equal(gc["end_node"], gc0["end_node"])
        for p in (0, 5, 11):
            assert np.array_equal(bits(g.path(p)), bits(ref.path(p)))
    for p in (0, 11):
        o = make_oracle(P, 21, 40 + p)
        assert o.solve(10 ** 6) == orc.SOLVED
        assert_same(chunked, p, o)


def test_se2_trees_beyond_the_lds_shadow_and_odd_headings(se2_golden):
    """Both trees grown to 2,000 nodes (the binary32 shadow holds 768: the rest is evaluated exactly, candidates come back from
    HBM); a start heading outside [-PI, PI] (the screen's heading formula does not apply: every node exactly)"""
    P = dict(se2_golden["gap"]["params"])
    box = [(8.0, 4.0, 10.0, 4.0), (8.0, 6.0, 10.0, 6.0), (8.0, 4.0, 8.0, 6.0), (10.0, 4.0, 10.0, 6.0)]
    P["segments"] = hexsegs(box)
    for flags in (0, capi.DEBUG_SE2_SMALL_LDS):
        g = make_gpu(P, 2, 5, 0, max_nodes=2000, debug_flags=flags)
        st = g.solve(10 ** 6)
        c, gc = g.counts(), g.goal_counts()
        assert (st == capi.ERR_NO_SOLUTION_FOUND).all() and (c["stop_reason"] == capi.STOP_NODES).all()
        assert int(max(c["nodes"].max(), gc["nodes"].max())) == 2000
        for p in range(2):
            o = make_oracle(P, 5, p, max_nodes=2000)
            assert o.solve(10 ** 6) == orc.NO_SOLUTION_FOUND
            assert_same(g, p, o, c, gc)
    Q = dict(se2_golden["soup256"]["params"])
    Q["start"] = [Q["start"][0], Q["start"][1], 4.0]
    g = make_gpu(Q, 3, 8, 0)
    assert (g.solve(10 ** 6) == capi.OK).all()
    for p in range(3):
        o = make_oracle(Q, 8, p)
        assert o.solve(10 ** 6) == orc.SOLVED
        assert_same(g, p, o)


def test_se2_crowded_cells_and_soups_beyond_the_lds_table(se2_golden):
    """A cell of the lookup grid that more than eight segments reach (its states meet every segment), and a soup of more than
    256 segments (the table stays in HBM / L2): planner runs and the stand-alone checks against the oracle"""
    P = dict(se2_golden["soup256"]["params"])
    base = segs_of(P)
    rng = np.random.default_rng(12)
    knot = np.column_stack([5.0 + rng.uniform(-0.05, 0.05, 14), 5.0 + rng.uniform(-0.05, 0.05, 14),
                            5.0 + rng.uniform(-0.05, 0.05, 14), 5.0 + rng.uniform(-0.05, 0.05, 14)])
    for segs in (np.vstack([base[:200], knot]), np.vstack([base, knot, base[:60] + 0.013])):
        Q = dict(P)
        Q["segments"] = hexsegs(segs)
        g = make_gpu(Q, 4, 31, 0)
        st = g.solve(200000)
        c, gc = g.counts(), g.goal_counts()
        for p in range(4):
            o = make_oracle(Q, 31, p)
            o.solve(200000)
            assert_same(g, p, o, c, gc)
        n = 1500
        a = np.column_stack([rng.uniform(4.5, 5.5, n), rng.uniform(4.5, 5.5, n), rng.uniform(-3, 3, n)])
        b = a + np.column_stack([rng.normal(0, 0.3, n), rng.normal(0, 0.3, n), rng.normal(0, 1.0, n)])
        m = g.check_motion(a, b)
        o = make_oracle(Q, 0, 0)
        assert 0.02 < m.mean() < 0.98
        for i in range(n):
            assert bool(m[i]) == o.check_motion(a[i], b[i])


# ------------------------------------------------------------------------------ frames
SE2_FRAMES = scenarios.SE2_FRAMES   # (the frames, and why each: oxmpl_amd/scenarios.py)


def se2_frame(P, scale, offset):
    """the scene P with (x, y) mapped to (x, y) * scale + offset: bounds, segment endpoints, start, goal, clearance, goal radius
    and max_distance (the last three scaled)"""
    t = lambda v: float(v) * scale + offset
    Q = dict(P)
    Q["bounds_xy"] = [[t(lo), t(hi)] for lo, hi in P["bounds_xy"]]
    Q["segments"] = hexsegs(segs_of(P) * scale + offset)
    Q["start"] = [t(P["start"][0]), t(P["start"][1]), P["start"][2]]
    Q["goal"] = [t(P["goal"][0]), t(P["goal"][1]), P["goal"][2]]
    Q["clearance"] = P["clearance"] * scale
    Q["goal_r"] = P["goal_r"] * scale
    Q["max_distance"] = P["max_distance"] * scale
    return Q


def _solve_in_cuts(g, budget, cut):
    done = 0
    while done < budget:
        step = min(cut, budget - done)
        g.solve(step)
        done += step


@pytest.mark.parametrize("scale,offset", SE2_FRAMES, ids=lambda v: "%g" % v)
@pytest.mark.parametrize("key", ["soup256", "gap"])
def test_se2_connect_frame_sweep(se2_golden, key, scale, offset):
    """Both golden scenes moved far from the origin, shrunk to 1e-12 and blown up beyond binary32's range: eight problems in one
    launch, the same without the segment grid, and the solve cut into launches of 37 iterations (every launch rebuilds the shadow
    and its magnitude from HBM) all equal the oracle bit for bit, solved or not"""
    P = se2_frame(se2_golden[key]["params"], scale, offset)
    budget, max_nodes, n = 1200, 400, 8
    oracles = []
    for p in range(n):
        o = make_oracle(P, 17, 300 + p, max_nodes=max_nodes)
        o.solve(budget)
        oracles.append(o)
    runs = [(0, budget), (capi.DEBUG_SE2_NO_SEGMENT_GRID, budget), (0, 37)]
    for flags, cut in runs:
        g = make_gpu(P, n, 17, 300, max_nodes=max_nodes, debug_flags=flags)
        _solve_in_cuts(g, budget, cut)
        c, gc = g.counts(), g.goal_counts()
        for p, o in enumerate(oracles):
            assert int(c["stop_reason"][p]) == o.stop_reason, (flags, cut, p)
            assert_same(g, p, o, c, gc)
        g.close()
    # the trees really grew (at 1e-12 the heading dominates every distance and the steps are tiny, but they are taken)
    assert max(o.num_nodes(0) + o.num_nodes(1) for o in oracles) > 20


def _states_around_clearance(segs, clearance, rng, n):
    """states whose distance to a segment is the clearance give or take an ulp or two of x or y: the checker's verdict flips
    among them"""
    out = []
    for j in rng.choice(len(segs), size=n, replace=len(segs) < n):
        x0, y0, x1, y1 = segs[j]
        u = float(rng.uniform(0.2, 0.8))
        mx, my = x0 + u * (x1 - x0), y0 + u * (y1 - y0)
        dx, dy = x1 - x0, y1 - y0
        ln = math.hypot(dx, dy)
        if not ln > 0.0:
            continue
        nx, ny = -dy / ln, dx / ln
        px, py = mx + nx * clearance, my + ny * clearance
        th = float(rng.uniform(-math.pi, math.pi))
        for k in (-2, -1, 0, 1, 2):
            xk = px
            for _ in range(abs(k)):
                xk = float(np.nextafter(xk, math.copysign(math.inf, k)))
            out.append((xk, py, th))
            yk = py
            for _ in range(abs(k)):
                yk = float(np.nextafter(yk, math.copysign(math.inf, k)))
            out.append((px, yk, th))
    return np.array(out, dtype=np.float64)


@pytest.mark.parametrize("scale,offset", SE2_FRAMES, ids=lambda v: "%g" % v)
def test_se2_checker_in_frames(se2_golden, scale, offset):
    """is_valid and check_motion of the segment grid (cell = (x - lo) G / w) against the oracle, in every frame: random states,
    random short motions, and states within an ulp or two of a segment's clearance"""
    P = se2_frame(se2_golden["soup256"]["params"], scale, offset)
    rng = np.random.default_rng(int(abs(math.log10(scale))) * 7 + 3)
    segs = segs_of(P)
    lo, hi = P["bounds_xy"][0][0], P["bounds_xy"][0][1]
    w = hi - lo
    n = 3000
    a = np.column_stack([lo + rng.uniform(0, 1, n) * w, lo + rng.uniform(0, 1, n) * w, rng.uniform(-math.pi, math.pi, n)])
    b = a + np.column_stack([rng.normal(0, 0.04, n) * w, rng.normal(0, 0.04, n) * w, rng.normal(0, 1.0, n)])
    edge = _states_around_clearance(segs, P["clearance"], rng, 150)
    edge_from = edge + np.column_stack([rng.normal(0, 0.02, len(edge)) * w, rng.normal(0, 0.02, len(edge)) * w, np.zeros(len(edge))])
    o = make_oracle(P, 0, 0)
    for flags in (0, capi.DEBUG_SE2_NO_SEGMENT_GRID):
        g = make_gpu(P, 1, 0, 0, debug_flags=flags)
        v, m = g.is_valid(a), g.check_motion(a, b)
        ve = g.is_valid(edge)
        me = g.check_motion(edge_from, edge)   # (a motion's last state is the edge state)
        want_v = np.array([o.is_valid(s) for s in a])
        want_m = np.array([o.check_motion(a[i], b[i]) for i in range(n)])
        want_ve = np.array([o.is_valid(s) for s in edge])
        want_me = np.array([o.check_motion(edge_from[i], edge[i]) for i in range(len(edge))])
        assert np.array_equal(v.astype(bool), want_v) and np.array_equal(m.astype(bool), want_m)
        assert np.array_equal(ve.astype(bool), want_ve) and np.array_equal(me.astype(bool), want_me)
        g.close()
    assert 0.2 < want_v.mean() < 0.98 and 0.05 < want_ve.mean() < 0.95   # both verdicts occur, at the edge too


def test_se2_arithmetic_in_frames_beyond_binary32():
    """se2_op_batch ops 0 and 1 (distance, SO(2) normalise / distance, interpolate) with (x, y) at and beyond binary32's range"""
    rng = np.random.default_rng(38)
    mags = [1e38, 3.4e38, float(np.float32(3.4028235e38)), 3.5e38, 1e39, 1e100]
    rows_a, rows_b = [], []
    for ma in mags:
        for mb in mags:
            for sa, sb in ((1, 1), (1, -1), (-1, 1)):
                th_a, th_b = rng.uniform(-4, 4, 2)
                jit = rng.uniform(0.5, 1.5, 4)
                rows_a.append((sa * ma * jit[0], ma * jit[1], th_a))
                rows_b.append((sb * mb * jit[2], -mb * jit[3], th_b))
    a, b = np.array(rows_a), np.array(rows_b)
    t = rng.uniform(0, 1, len(a))
    t[:4] = [0.0, 1.0, 0.5, 1e-300]
    out0 = capi.se2_op_batch(0, a, b)
    out1 = capi.se2_op_batch(1, a, b, t)
    L = orc.lib()
    for i in range(len(a)):
        assert bits(out0[i, 0:1])[0] == bits(np.array([orc.se2_distance(a[i], b[i])]))[0], i
        assert bits(out0[i, 1:2])[0] == bits(np.array([L.orc_so2_normalise(a[i, 2])]))[0]
        assert bits(out0[i, 2:3])[0] == bits(np.array([L.orc_so2_distance(a[i, 2], b[i, 2])]))[0]
        assert np.array_equal(bits(out1[i]), bits(orc.se2_interpolate(a[i], b[i], float(t[i])))), i


def _se2_res(P):
    (x0, x1), (y0, y1) = P["bounds_xy"]
    acc = 0.0
    for w in (x1 - x0, y1 - y0):
        acc = acc + w * w
    return (math.sqrt(acc) + 0.5 * math.pi) * P["fraction"] * 0.1   # extent_xy + PI / 2, times the fraction, times 0.1


def _host_adv_steps(max_distance, res):
    """oxhip_api.hip's rule, restated: an Advanced extend's step count is the constant ceil(max_distance / res) when that ratio
    is farther than 1e-6 from an integer; returns adv_steps, 0 = none"""
    r = max_distance / res
    c = math.ceil(r)
    gap = min(r - (c - 1.0), c - r)
    return int(c) if math.isfinite(r) and 1.0 <= c < 4294967295.0 and gap > 1e-6 else 0


def test_se2_connect_known_step_count_boundary(se2_golden):
    """The constant step count of an Advanced extend (adv_steps, taken when (mag + |qx| + |qy| + 4 + max_distance) 2^-45 <
    adv_slack).  (1) max_distance / res just beyond and just inside the host's 1e-6 gap from an integer, on both sides of it, at
    offsets where that condition holds for every query, for part of them and for none: parity with the oracle (which always takes
    ceil(distance / res)) around the boundary of the rule, in one launch and in launches of 37 iterations.  (2) Far from the origin
    (1e10, -3e10) the rounding of an Advanced motion's length exceeds the gap, so ceil(distance / res) really differs from
    adv_steps for many motions, and with a clearance of 0.02 (less than a step) the states a motion check tests decide its verdict:
    a kernel that took the constant there would part from the oracle."""
    base = se2_golden["soup256"]["params"]
    res = _se2_res(base)
    k, budget = 6, 1200

    def run(P, n, cuts):
        assert _se2_res(P) == res
        oracles = []
        for p in range(n):
            o = make_oracle(P, 29, 70 + p, max_nodes=500)
            o.solve(budget)
            oracles.append(o)
        for cut in cuts:
            gpu = make_gpu(P, n, 29, 70, max_nodes=500)
            _solve_in_cuts(gpu, budget, cut)
            c, gc = gpu.counts(), gpu.goal_counts()
            for p, o in enumerate(oracles):
                assert int(c["stop_reason"][p]) == o.stop_reason
                assert_same(gpu, p, o, c, gc)
            gpu.close()
        return oracles

    host = []
    for g in (1.25e-6, -1.25e-6, 0.8e-6, -0.8e-6):
        md = (k + g) * res
        host.append(_host_adv_steps(md, res))
        # mag (the goal tree starts at offset + 9.5) + |qx| + |qy| spans 3 offset + [9.5, 30]: the condition holds for every
        # query below T - 10, for part of them at T - 6.5, for none above T - 3.2
        T = (0.5 * abs(g) * res * 2.0 ** 45 - 4.0 - md) / 3.0
        for off in (0.5 * T, T - 6.5, 1.5 * T):
            run(se2_frame(dict(base, max_distance=md), 1.0, float(round(off))), 6, (budget, 37))   # (integral: widths stay 10)
    assert host == [k + 1, k, 0, 0]   # (the construction: the constant just beyond the gap on either side of k, none inside it)
    # (2) a thin clearance far out
    differ = 0
    for g in (1.25e-6, -1.25e-6):
        md = (k + g) * res
        steps = _host_adv_steps(md, res)
        for off in (1.0e10, -3.0e10):
            for o in run(se2_frame(dict(base, max_distance=md, clearance=0.02), 1.0, off), 8, (budget,)):
                for w in (0, 1):
                    st, par = o.tree(w)
                    for i in range(1, len(par)):
                        d = orc.se2_distance(st[par[i]], st[i])
                        differ += abs(d - md) < 1e-3 and math.ceil(d / res) != steps
    assert differ > 0   # Advanced motions whose step count is not the constant were taken (and many more were tested)
