"""GPU: PRM over SO(3) (prm_so3.hip) against the CPU checker tests/golden/make_golden_prm_so3.py, bit for bit, and against an
independent device path (oxhip_so3_op_batch distances + oxhip_rrt_batch_check_motion on an SO(3) batch) on a large roadmap."""
import json
import math
import os
import struct
import sys

import numpy as np
import pytest

from oxmpl_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_prm_so3 as gp  # noqa: E402
import make_golden_so3 as g3  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURE = [0.0, 0.0, 0.0, 1.0, math.pi]
PIO2 = 1.57079632679489655800e+00
STATUS = {capi.OK: "solved", capi.ERR_NO_SOLUTION_FOUND: "no_solution", capi.ERR_INVALID_START_STATE: "invalid_start",
          capi.ERR_UNSAMPLED_STATE_SPACE: "unsampled"}


def _bits(rows):
    return [["%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0] for v in row] for row in rows]


def _make(sc, radius=None, max_milestones=None, **kw):
    bounds = FIXTURE if sc["bounds"] is None else list(sc["bounds"][0]) + [sc["bounds"][1]]
    args = dict(lvs_fraction=sc["fraction"], max_samples=sc["max_samples"], seed=sc["seed"], stream=sc["stream"], space=capi.SPACE_SO3)
    args.update(kw)
    g = capi.PRMRoadmap(4, bounds, sc["radius"] if radius is None else radius,
                        sc["max_milestones"] if max_milestones is None else max_milestones, **args)
    if sc["cones"]:
        g.set_spheres([c for c, _ in sc["cones"]], [r for _, r in sc["cones"]])
    start, target, goal_r = sc["queries"][0]
    g.setup(start, target, goal_r)
    return g


def _edges(g):
    states, off, nbrs = g.roadmap()
    return states, [[int(v) for v in nbrs[int(off[i]):int(off[i + 1])]] for i in range(len(states))]


def _query(g):
    st, path = g.solve()
    sc, gi = g.query_sets()
    return STATUS.get(st, st), [int(v) for v in sc], [int(v) for v in gi], path


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "prm_so3_golden.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", ["fixture", "bounded", "wide_radius", "tiny_radius", "degenerate", "sample_cap"])
def test_golden_scenes_bit_for_bit(golden, name):
    sc, want = gp.scenes()[name], golden[name]["run"]
    g = _make(sc)
    g.construct_roadmap()
    n, entries, n_samples = g.sizes()
    assert (n, n_samples) == (want["n"], want["n_samples"])
    states, edges = _edges(g)
    assert _bits(states) == want["states"]
    assert edges == want["edges"]
    for k, (q, wq) in enumerate(zip(sc["queries"], want["queries"])):
        if k:
            g.set_problem(*q)   # multi-query use: the roadmap is kept
        status, s_conn, g_idx, path = _query(g)
        assert status == wq["status"], (k, status)
        assert s_conn == wq["start_connections"] and g_idx == wq["goal_indices"], k
        assert _bits(path) == wq["path"], k
    g.close()


def test_set_problem_equals_a_fresh_setup():
    sc = gp.scenes()["bounded"]
    a = _make(sc)
    a.construct_roadmap()
    a.solve()
    a.set_problem(*sc["queries"][1])
    b = _make(dict(sc, queries=sc["queries"][1:]))
    b.construct_roadmap()
    ra, rb = _query(a), _query(b)
    assert ra[:3] == rb[:3] and np.array_equal(ra[3].view(np.uint64), rb[3].view(np.uint64))


def test_python_prm_on_the_fixture_at_16384_milestones():
    from oxmpl_amd.base import ProblemDefinition, SO3ConeValidityChecker, SO3State, SO3StateSpace
    from oxmpl_amd.geometric import PRM

    class Goal:
        def __init__(self, target, radius):
            self.target, self.radius = target, radius

    start = g3.quaternion_from_axis_angle([0.0, 1.0, 0.0], g3.PI / 2.0)
    target = g3.quaternion_from_axis_angle([0.0, 1.0, 0.0], -g3.PI / 2.0)
    goal_r = 10.0 * (g3.PI / 180.0)
    cone = ([0.0, 0.0, 0.0, 1.0], 44.9 * (g3.PI / 180.0))
    pd = ProblemDefinition.from_so3(SO3StateSpace(), SO3State(*start), Goal(SO3State(*target), goal_r))
    planner = PRM(5.0, 0.5, pd, max_milestones=16384, seed=1)
    planner.setup(SO3ConeValidityChecker([(SO3State(*cone[0]), cone[1])]))
    planner.construct_roadmap()
    states, _, _ = planner.get_roadmap()
    assert len(states) == 16384 and isinstance(states[0], SO3State)
    path = planner.solve(5.0)
    rows = [s.values for s in path.states]
    assert isinstance(path.states[0], SO3State) and len(rows) >= 2
    assert g3.distance(rows[0], start) < 1e-9                       # prm_so3ss_tests.rs assertions
    assert g3.distance(rows[-1], target) <= goal_r
    assert g3.is_so3_path_valid(rows, g3.Cones([cone]), 0.05)


def _independent_edges(states, radius, cones, fraction):
    """every pair with oxhip_so3_op_batch distance < r, then oxhip_rrt_batch_check_motion (from = the newer milestone)"""
    n = len(states)
    js, is_ = [], []
    for j0 in range(1, n, 512):
        j1 = min(n, j0 + 512)
        jj, ii = np.nonzero(np.tril(np.ones((j1 - j0, j1), dtype=bool), k=j0 - 1))
        jj = jj + j0
        d = capi.so3_op_batch(0, states[jj], states[ii])
        keep = d < radius
        js.append(jj[keep])
        is_.append(ii[keep])
    js, is_ = np.concatenate(js), np.concatenate(is_)
    b = capi.RRTBatch(4, FIXTURE, 0.5, 0.0, 1, max_nodes=16, lvs_fraction=fraction, space=capi.SPACE_SO3)
    b.set_spheres([c for c, _ in cones], [r for _, r in cones])
    ok = np.concatenate([b.check_motion(states[js[k:k + 4000000]], states[is_[k:k + 4000000]]).astype(bool)
                         for k in range(0, len(js), 4000000)])
    b.close()
    u, v = np.concatenate([js[ok], is_[ok]]), np.concatenate([is_[ok], js[ok]])
    order = np.lexsort((v, u))
    return u[order], v[order], len(js)


@pytest.mark.parametrize("n,radius", [(2048, 0.5), (16384, 0.5)])
def test_large_roadmap_against_an_independent_device_path(n, radius):
    sc = dict(gp.scenes()["fixture"], max_milestones=n, radius=radius, seed=21)
    g = _make(sc)
    g.construct_roadmap()
    states, off, nbrs = g.roadmap()
    assert len(states) == n
    u, v, n_cand = _independent_edges(states, radius, sc["cones"], sc["fraction"])
    assert g.last_timing()["candidates"] == n_cand
    assert np.array_equal(off.astype(np.int64), np.searchsorted(u, np.arange(n + 1)))
    assert np.array_equal(nbrs.astype(np.int64), v)
    # the milestones and the sample count are the checker's sampler, word for word
    rng = g3.mg.ChaCha12Rng(sc["seed"], sc["stream"])
    cones, ms, calls = g3.Cones(sc["cones"]), [], 0
    while len(ms) < 2048:
        q = g3.sample_uniform(rng, [0.0, 0.0, 0.0, 1.0], g3.PI)
        calls += 1
        if cones.is_valid(q):
            ms.append(q)
    assert _bits(states[:2048]) == _bits(ms)
    if n == 2048:
        assert g.sizes()[2] == calls
    g.close()


def test_rounds_and_sample_cuts_give_the_same_roadmap():
    sc = dict(gp.scenes()["bounded"], max_milestones=10000)
    one = _make(sc)
    one.construct_roadmap()
    s1, e1 = _edges(one)
    rounds = _make(sc, timeout=1e6)          # finite timeout: doubling rounds 4096, 8192, 10000
    rounds.construct_roadmap()
    s2, e2 = _edges(rounds)
    assert np.array_equal(s1.view(np.uint64), s2.view(np.uint64)) and e1 == e2
    assert one.sizes() == rounds.sizes()
    _, _, total = one.sizes()
    for cap in (1, 777, total // 2):
        cut = _make(sc, max_samples=cap)
        cut.construct_roadmap()
        n, _, ns = cut.sizes()
        assert ns == cap
        s3, e3 = _edges(cut)
        assert np.array_equal(s3.view(np.uint64), s1[:n].view(np.uint64))
        assert e3 == [[i for i in e if i < n] for e in e1[:n]]
        cut.close()


def _bands(r):
    if not (r <= PIO2):
        return -1.0, -1.0
    hi = math.cos(r * (1.0 - 2.0 ** -40)) + 2.0 ** -50
    lo = min(math.cos(r * (1.0 + 2.0 ** -40)) - 2.0 ** -50, 1.0 - 1e-9)
    return lo, hi


def _checker(sc, radius, n):
    rm = gp.prm_construct(sc["bounds"], radius, sc["fraction"], g3.Cones(sc["cones"]), sc["seed"], sc["stream"], n, sc["max_samples"])
    return rm["states"], rm["edges"]


def test_radius_at_a_pair_distance_and_one_ulp_either_side():
    sc = gp.scenes()["fixture"]
    states, _ = _checker(sc, 0.0, 40)
    # the pair (j, i) whose motion is valid and whose distance is nearest 0.3
    best = min(((abs(g3.distance(states[j], states[i]) - 0.3), j, i) for j in range(40) for i in range(j)
                if g3.check_motion(g3.Cones(sc["cones"]), sc["fraction"], states[j], states[i])))
    _, j, i = best
    d = g3.distance(states[j], states[i])
    ad = abs(g3.dot(states[j], states[i]))
    for r in (d, math.nextafter(d, 0.0), math.nextafter(d, math.inf)):
        lo, hi = _bands(r)
        assert lo <= ad <= hi                      # decided by the exact distance, not by a band
        _, want = _checker(sc, r, 40)
        assert (i in want[j]) == (d < r)
        g = _make(sc, radius=r, max_milestones=40)
        g.construct_roadmap()
        assert _edges(g)[1] == want, r
        g.close()


@pytest.mark.parametrize("radius", [0.0, -1.0, PIO2, math.nextafter(PIO2, math.inf), math.inf])
def test_radius_edge_cases(radius):
    sc = gp.scenes()["fixture"]
    n = 48
    g = _make(sc, radius=radius, max_milestones=n)
    g.construct_roadmap()
    states, edges = _edges(g)
    ref_states, want = _checker(sc, radius, n)
    assert _bits(states) == _bits(ref_states) and edges == want
    if radius > PIO2:   # every pair is a candidate
        assert g.last_timing()["candidates"] == n * (n - 1) // 2
    if radius <= 0.0:
        assert all(e == [] for e in edges)
    g.close()


def test_a_fully_forbidden_space_is_unsampled_and_boxes_are_refused():
    sc = dict(gp.scenes()["fixture"], cones=[([0.0, 0.0, 0.0, 1.0], PIO2)], max_samples=20000)
    g = _make(sc)
    g.construct_roadmap()
    assert g.sizes()[0] == 0 and g.sizes()[2] == 20000
    assert g.solve()[0] == capi.ERR_UNSAMPLED_STATE_SPACE
    with pytest.raises(capi.OxhipError) as ei:
        g.set_boxes([[0.0, 0.0, 0.0, 0.0]], [[1.0, 1.0, 1.0, 1.0]])
    assert ei.value.status == capi.ERR_BAD_ARG
    g.close()
