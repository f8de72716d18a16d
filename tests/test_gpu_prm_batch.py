"""GPU: a batch of PRM queries on one roadmap (oxhip_prm_solve_batch, prm_batch.hip) -- start connections, goal test,
breadth-first search and path extraction on the device -- against what set_problem + solve return on the same handle, the CPU
oracle (oracle/prm_oracle.c), the golden files and the pure-Python checker of the SO(3) PRM.  Every comparison is bit for bit:
statuses, both query sets, the goal milestone reached and every path row."""
import json
import math
import os
import sys

import numpy as np
import pytest

from helpers import unhex, bits, params_spheres, params_boxes, is_path_valid
from prm_helpers import make_oracle_prm, STATUS_NAME

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_prm_so3 as gp3  # noqa: E402
import make_golden_so3 as g3  # noqa: E402

pytestmark = pytest.mark.gpu

from oxmpl_amd import capi, scenarios  # noqa: E402
from oracle import oracle_py as orc  # noqa: E402

SEED = 20261016
START_ROW = 0xFFFFFFFF
FIXTURE = [0.0, 0.0, 0.0, 1.0, math.pi]


def _golden(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return json.load(f)


def make_gpu_prm(P, **kw):
    args = dict(max_milestones=P["max_milestones"], lvs_fraction=P["fraction"], seed=P["seed"], stream=P["stream"],
                max_samples=0 if P["max_samples"] >= 10 ** 9 else P["max_samples"])
    args.update(kw)
    g = capi.PRMRoadmap(P["dim"], P["bounds"], P["radius"], **args)
    if P["spheres"]:
        g.set_spheres(*params_spheres(P))
    if P["boxes"]:
        g.set_boxes(*params_boxes(P))
    return g


def make_so3_prm(sc, **kw):
    bounds = FIXTURE if sc["bounds"] is None else list(sc["bounds"][0]) + [sc["bounds"][1]]
    args = dict(lvs_fraction=sc["fraction"], max_samples=sc["max_samples"], seed=sc["seed"], stream=sc["stream"], space=capi.SPACE_SO3)
    args.update(kw)
    g = capi.PRMRoadmap(4, bounds, sc["radius"], sc["max_milestones"], **args)
    if sc["cones"]:
        g.set_spheres([c for c, _ in sc["cones"]], [r for _, r in sc["cones"]])
    return g


class Batch:
    """one solve_batch and everything its getters return, with the invariants that tie them together"""

    def __init__(self, g, starts, goals, radii, **kw):
        self.starts = np.asarray(starts, dtype=np.float64).reshape(len(radii), g.dim)
        self.status = g.solve_batch(starts, goals, radii, **kw).copy()
        r = g.batch_results()
        assert np.array_equal(self.status, r["status"])
        self.len, self.goal, self.ns, self.ng = r["path_len"], r["goal_node"], r["n_start"], r["n_goal"]
        self.off, self.nodes, self.rows = g.batch_paths()
        self.timing = g.batch_last_timing()
        q = len(radii)
        assert len(self.status) == q and len(self.off) == q + 1 and int(self.off[0]) == 0
        assert np.array_equal(np.diff(self.off.astype(np.int64)), self.len.astype(np.int64))
        assert len(self.nodes) == int(self.off[-1]) and self.rows.shape == (int(self.off[-1]), g.dim)
        ok = self.status == capi.OK
        assert np.all(self.len[~ok] == 0) and np.all(self.goal[~ok] == -1) and np.all(self.len[ok] >= 2)
        bad = (self.status == capi.ERR_INVALID_START_STATE) | (self.status == capi.ERR_TIMEOUT)
        assert np.all(self.ns[bad] == 0) and np.all(self.ng[bad] == 0)
        assert set(np.unique(self.status)) <= {capi.OK, capi.ERR_NO_SOLUTION_FOUND, capi.ERR_INVALID_START_STATE, capi.ERR_TIMEOUT}

    def path(self, q):
        return self.rows[int(self.off[q]):int(self.off[q + 1])]

    def path_nodes(self, q):
        return self.nodes[int(self.off[q]):int(self.off[q + 1])]

    def check_rows_are_milestones(self, milestones):
        """row 0 of every path is the start state, every other row the milestone its node index names, the last the goal milestone"""
        for q in np.nonzero(self.status == capi.OK)[0]:
            nd, rows = self.path_nodes(q), self.path(q)
            assert nd[0] == START_ROW and np.array_equal(bits(rows[0]), bits(self.starts[q]))
            assert np.array_equal(bits(rows[1:]), bits(milestones[nd[1:]]))
            assert int(nd[-1]) == int(self.goal[q])

    def same_as(self, other):
        for a, b in ((self.status, other.status), (self.len, other.len), (self.goal, other.goal), (self.ns, other.ns), (self.ng, other.ng),
                     (self.off, other.off), (self.nodes, other.nodes), (bits(self.rows), bits(other.rows))):
            assert np.array_equal(a, b)


def assert_batch_equals_single_solves(g, B, starts, goals, radii, sets_every=1):
    """query by query what set_problem + solve return on the same handle"""
    for q in range(len(radii)):
        g.set_problem(starts[q], goals[q], radii[q])
        st, path = g.solve()
        assert st == B.status[q], q
        assert path.shape == B.path(q).shape and np.array_equal(bits(path), bits(B.path(q))), q
        sc, gi = g.query_sets()
        assert (len(sc), len(gi)) == (int(B.ns[q]), int(B.ng[q])), q
        if q % sets_every == 0:
            bsc, bgi = g.batch_query_sets(q)
            assert np.array_equal(sc, bsc) and np.array_equal(gi, bgi), q


def oracle_loop(o, starts, goals, radii):
    """the reference for a batch: OraclePRM.set_problem + solve per query -> list of (status, start_connections, goal_indices, path)"""
    out = []
    for q in range(len(radii)):
        o.set_problem(starts[q], goals[q], radii[q])
        st = o.solve()
        if st == capi.ERR_INVALID_START_STATE:
            out.append((st, np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros((0, o.dim))))
        else:
            out.append((st, o.start_connections().copy(), o.goal_indices().copy(), o.path().copy()))
    return out


def assert_batch_equals_oracle(g, B, answers, sets_every=1):
    for q, (st, sc, gi, path) in enumerate(answers):
        assert B.status[q] == st, q
        assert (int(B.ns[q]), int(B.ng[q])) == (len(sc), len(gi)), q
        assert path.shape == B.path(q).shape and np.array_equal(bits(path), bits(B.path(q))), q
        if q % sets_every == 0:
            bsc, bgi = g.batch_query_sets(q)
            assert np.array_equal(sc, bsc) and np.array_equal(gi, bgi), q
        if st == capi.OK:
            assert int(B.goal[q]) in set(int(v) for v in gi), q


def mix(answers):
    st = [a[0] for a in answers]
    return st.count(capi.OK), st.count(capi.ERR_NO_SOLUTION_FOUND), st.count(capi.ERR_INVALID_START_STATE)


def seeded_queries(n, dim, r_lo, r_hi, lo=0.0, hi=10.0):
    """starts, goal centres uniform in [lo, hi)^dim, goal radii uniform in [r_lo, r_hi): drawn in that order"""
    rng = np.random.default_rng(SEED)
    starts = rng.uniform(lo, hi, size=(n, dim))
    goals = rng.uniform(lo, hi, size=(n, dim))
    radii = rng.uniform(r_lo, r_hi, size=n) if r_hi > r_lo else np.full(n, r_lo)
    return starts, goals, radii


# ------------------------------------------------------------------------------------------------ 1. the recorded queries
@pytest.mark.parametrize("fname,key", [("prm_golden.json", k) for k in ("wall", "r3", "r6", "sample_cap")]
                         + [("prm_knn_golden.json", k) for k in ("wall_k6", "r3_k10", "r6_k8", "wall_k1")])
def test_recorded_queries_of_the_rn_golden_scenes_in_one_batch(fname, key):
    rec = _golden(fname)[key]
    P, R = rec["params"], rec["run"]
    qs = R["queries"]
    g = make_gpu_prm(P, knn_k=P.get("knn_k", 0))
    g.setup(qs[0]["start"], qs[0]["goal_c"], qs[0]["goal_r"])
    g.construct_roadmap()
    starts, goals, radii = [q["start"] for q in qs], [q["goal_c"] for q in qs], [q["goal_r"] for q in qs]
    B = Batch(g, starts, goals, radii)
    B.check_rows_are_milestones(g.roadmap()[0])
    for k, q in enumerate(qs):
        assert STATUS_NAME[int(B.status[k])] == q["status"], k
        want = np.array([[unhex(v) for v in row] for row in q["path"]]).reshape(-1, P["dim"])
        assert want.shape == B.path(k).shape and np.array_equal(bits(want), bits(B.path(k))), k
        sc, gi = g.batch_query_sets(k)
        assert list(sc) == q["start_connections"] and list(gi) == q["goal_indices"], k
        if q["status"] == "solved":
            assert int(B.goal[k]) in q["goal_indices"]
    assert_batch_equals_single_solves(g, B, starts, goals, radii)
    g.close()


@pytest.mark.parametrize("name", ["fixture", "bounded", "wide_radius", "tiny_radius", "degenerate", "sample_cap"])
def test_recorded_queries_of_the_so3_golden_scenes_in_one_batch(name):
    sc, want = gp3.scenes()[name], _golden("prm_so3_golden.json")[name]["run"]
    g = make_so3_prm(sc)
    g.setup(*sc["queries"][0])
    g.construct_roadmap()
    starts, goals, radii = [q[0] for q in sc["queries"]], [q[1] for q in sc["queries"]], [q[2] for q in sc["queries"]]
    B = Batch(g, starts, goals, radii)
    B.check_rows_are_milestones(g.roadmap()[0])
    for k, wq in enumerate(want["queries"]):
        assert STATUS_NAME[int(B.status[k])] == wq["status"], k
        w = np.array([[unhex(v) for v in row] for row in wq["path"]]).reshape(-1, 4)
        assert w.shape == B.path(k).shape and np.array_equal(bits(w), bits(B.path(k))), k
        s_conn, g_idx = g.batch_query_sets(k)
        assert list(s_conn) == wq["start_connections"] and list(g_idx) == wq["goal_indices"], k
    assert_batch_equals_single_solves(g, B, starts, goals, radii)
    g.close()


# ------------------------------------------------------------------------------------------------ 2. the batch golden file
@pytest.mark.parametrize("scene", ["wall", "r6", "fixture"])
def test_batch_golden_scenes(scene):
    rec = _golden("prm_batch_golden.json")[scene]
    qs = rec["queries"]
    starts = [[unhex(v) for v in q["start"]] for q in qs]
    goals = [[unhex(v) for v in q["goal_c"]] for q in qs]
    radii = [unhex(q["goal_r"]) for q in qs]
    if rec["space"] == "so3":
        sc = gp3.scenes()["fixture"]
        g = make_so3_prm(sc)
    else:
        g = make_gpu_prm(_golden("prm_golden.json")[scene]["params"])
    g.setup(starts[0], goals[0], radii[0])
    g.construct_roadmap()
    assert g.sizes()[0] == rec["n"] and len(qs) == 32
    B = Batch(g, starts, goals, radii)
    B.check_rows_are_milestones(g.roadmap()[0])
    for k, q in enumerate(qs):
        assert STATUS_NAME[int(B.status[k])] == q["status"], k
        want_sets = (0, 0) if q["status"] == "invalid_start" else (q["n_start"], q["n_goal"])
        assert (int(B.ns[k]), int(B.ng[k])) == want_sets and int(B.goal[k]) == q["goal_node"], k
        want = np.array([[unhex(v) for v in row] for row in q["path"]]).reshape(-1, g.dim)
        assert want.shape == B.path(k).shape and np.array_equal(bits(want), bits(B.path(k))), k
    g.close()


# ------------------------------------------------------------------------------------------------ 3. / 5. R^6, 4,096 milestones
def _r6_params(n, radius, seed=11, stream=5, n_spheres=16):
    """(as tests/test_gpu_prm.py)"""
    rng = np.random.default_rng(1234)
    centres = rng.uniform(1.0, 9.0, size=(n_spheres, 6))
    radii = rng.uniform(3.0, 4.5, size=n_spheres)
    return dict(dim=6, bounds=[(0.0, 10.0)] * 6, radius=radius, fraction=0.05, seed=seed, stream=stream,
                max_milestones=n, max_samples=10 ** 9, boxes=[],
                spheres=[(list(map(float, c)), float(r)) for c, r in zip(centres, radii)])


@pytest.fixture(scope="module")
def r6_4096():
    P = _r6_params(4096, 3.0)
    g, o = make_gpu_prm(P), make_oracle_prm(P)
    for x in (g, o):
        x.setup([2.0] * 6, [8.0] * 6, 2.5)
    g.construct_roadmap()
    o.construct_roadmap(4096)
    starts, goals, radii = seeded_queries(256, 6, 1.5, 2.5)
    answers = oracle_loop(o, starts, goals, radii)
    yield g, starts, goals, radii, answers
    g.close()


def test_r6_4096_milestones_256_queries_against_the_oracle(r6_4096):
    g, starts, goals, radii, answers = r6_4096
    assert mix(answers) == (112, 94, 50)                       # the oracle's own mix: not an all-refused batch
    assert max(len(a[3]) for a in answers) == 11
    B = Batch(g, starts, goals, radii)
    B.check_rows_are_milestones(g.roadmap()[0])
    assert_batch_equals_oracle(g, B, answers)


def test_results_do_not_depend_on_chunking_order_or_company(r6_4096):
    g, starts, goals, radii, answers = r6_4096
    ref = Batch(g, starts, goals, radii)
    assert ref.timing["rounds"] == 1
    for chunk, rounds in ((1, 256), (7, 37), (64, 4), (0, 1)):
        B = Batch(g, starts, goals, radii, chunk_queries=chunk)
        assert B.timing["rounds"] == rounds
        B.same_as(ref)
    for q in range(16):                                        # each query as a batch of one
        one = Batch(g, starts[q:q + 1], goals[q:q + 1], radii[q:q + 1])
        assert one.status[0] == ref.status[q] and one.goal[0] == ref.goal[q] and (one.ns[0], one.ng[0]) == (ref.ns[q], ref.ng[q])
        assert np.array_equal(one.nodes, ref.path_nodes(q)) and np.array_equal(bits(one.rows), bits(ref.path(q)))
    rev = Batch(g, starts[::-1], goals[::-1], radii[::-1])
    for a, b in ((rev.status, ref.status), (rev.len, ref.len), (rev.goal, ref.goal), (rev.ns, ref.ns), (rev.ng, ref.ng)):
        assert np.array_equal(a[::-1], b)
    for q in range(256):
        assert np.array_equal(rev.path_nodes(255 - q), ref.path_nodes(q)) and np.array_equal(bits(rev.path(255 - q)), bits(ref.path(q)))


# ------------------------------------------------------------------------------------------------ 4. config 5 at full size
def test_config5_50000_milestones_1024_queries_against_the_oracle():
    sc = scenarios.config5()
    g = scenarios.make_prm(sc, 50000)
    g.construct_roadmap()
    o = orc.OraclePRM(6, sc["bounds"], sc["connection_radius"], lvs_fraction=sc["lvs_fraction"], seed=42, stream=0)
    o.set_spheres(*sc["spheres"])
    o.setup(sc["start"], sc["goal_centre"], sc["goal_radius"])
    o.construct_roadmap(50000)
    starts, goals, radii = seeded_queries(1024, 6, 1.5, 2.5)
    answers = oracle_loop(o, starts, goals, radii)
    assert mix(answers) == (918, 20, 86)
    lens = sorted(len(a[3]) for a in answers if a[0] == capi.OK)
    assert (lens[0], lens[-1]) == (2, 15)
    B = Batch(g, starts, goals, radii)
    print("config 5, 50,000 milestones, 1,024 queries: phases (ms) flags / search / paths / copies %s, rounds %d"
          % (["%.3f" % v for v in B.timing["phase_ms"]], B.timing["rounds"]))
    B.check_rows_are_milestones(g.roadmap()[0])
    assert_batch_equals_oracle(g, B, answers, sets_every=16)
    g.close()


# ------------------------------------------------------------------------------------------------ 6. ties
@pytest.mark.parametrize("n,radius,n_queries,goal_r,edge_entries", [(2048, 1.0, 128, 2.0, 119974), (2048, 3.0, 128, 0.3, 895460),
                                                                     (256, float("inf"), 64, 2.0, 65280)])
def test_ties_between_candidate_parents(n, radius, n_queries, goal_r, edge_entries):
    """open R^2: many goal milestones per query, hundreds of candidate parents per node, and the complete graph -- where a wrong
    minimum or a wrong level order shows"""
    P = dict(dim=2, bounds=[(0.0, 10.0), (0.0, 10.0)], radius=radius, fraction=0.05, seed=3, stream=2, max_milestones=n,
             max_samples=10 ** 9, boxes=[], spheres=[])
    g, o = make_gpu_prm(P), make_oracle_prm(P)
    for x in (g, o):
        x.setup([1.0, 1.0], [9.0, 9.0], 1.0)
    g.construct_roadmap()
    o.construct_roadmap(n)
    assert g.sizes()[:2] == (n, edge_entries)
    starts, goals, radii = seeded_queries(n_queries, 2, goal_r, goal_r)
    answers = oracle_loop(o, starts, goals, radii)
    assert mix(answers) == (n_queries, 0, 0)                   # all solved
    B = Batch(g, starts, goals, radii)
    B.check_rows_are_milestones(g.roadmap()[0])
    assert_batch_equals_oracle(g, B, answers)
    if math.isinf(radius):                                     # every path is [start, lowest-index goal milestone]
        for q, (_, sc, gi, path) in enumerate(answers):
            assert list(B.path_nodes(q)) == [START_ROW, int(gi.min())]
    g.close()


# ------------------------------------------------------------------------------------------------ 7. every status by construction
def test_every_status_by_construction():
    P = dict(dim=2, bounds=[(0.0, 10.0), (0.0, 10.0)], radius=0.6, fraction=0.05, seed=5, stream=1, max_milestones=1200,
             max_samples=10 ** 9, boxes=[], spheres=[([5.0, 5.0], 1.0)])
    g, o = make_gpu_prm(P), make_oracle_prm(P)
    with pytest.raises(capi.OxhipError) as ei:                 # before setup
        g.solve_batch([[1.0, 1.0]], [[9.0, 9.0]], [1.0])
    assert ei.value.status == capi.ERR_PLANNER_UNINITIALISED
    for x in (g, o):
        x.setup([1.0, 1.0], [9.0, 9.0], 1.0)
    for call in (lambda: g.solve_batch([[1.0, 1.0]], [[9.0, 9.0]], [1.0]), g.batch_results, g.batch_paths):   # empty roadmap
        with pytest.raises(capi.OxhipError) as ei:
            call()
        assert ei.value.status == capi.ERR_UNSAMPLED_STATE_SPACE
    g.construct_roadmap()
    o.construct_roadmap(1200)
    ms = g.roadmap()[0]
    empty = Batch(g, np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0))      # n_queries = 0
    assert len(empty.status) == 0 and len(empty.nodes) == 0 and empty.timing["rounds"] == 0
    m7 = ms[7]
    queries = [([5.2, 5.1], [9.0, 9.0], 1.0),                  # start inside the sphere
               ([1.0, 1.0], [9.0, 9.0], 0.0),                  # goal radius 0 away from any milestone
               ([100.0, 100.0], [9.0, 9.0], 1.0),              # start farther than the radius from everything
               (list(m7), list(m7), 0.0),                      # the start connection m7 is itself the goal milestone
               ([1.0, 1.0], [9.0, 9.0], 1.0)]
    starts, goals, radii = [q[0] for q in queries], [q[1] for q in queries], [q[2] for q in queries]
    answers = oracle_loop(o, starts, goals, radii)
    assert [a[0] for a in answers] == [capi.ERR_INVALID_START_STATE, capi.ERR_NO_SOLUTION_FOUND, capi.ERR_NO_SOLUTION_FOUND, capi.OK, capi.OK]
    assert len(answers[1][2]) == 0 and len(answers[1][1]) > 0 and len(answers[2][1]) == 0 and len(answers[2][2]) > 0
    assert len(answers[3][3]) == 2
    B = Batch(g, starts, goals, radii)
    assert_batch_equals_oracle(g, B, answers)
    assert list(B.path_nodes(3)) == [START_ROW, 7]
    with pytest.raises(capi.OxhipError) as ei:                 # what set_problem refuses, the batch refuses
        g.solve_batch([[float("nan"), 1.0]], [[9.0, 9.0]], [1.0])
    assert ei.value.status == capi.ERR_BAD_ARG
    g.close()


def test_search_runs_dry_on_a_disconnected_roadmap():
    """the wall scene with a radius so small that the roadmap falls apart; start and goal on opposite sides of the wall"""
    P = dict(_golden("prm_golden.json")["wall"]["params"], radius=0.22, max_milestones=1500)
    g, o = make_gpu_prm(P), make_oracle_prm(P)
    starts, goals, radii = [[1.0, 5.0], [9.0, 5.0]], [[9.0, 5.0], [1.0, 5.0]], [0.5, 0.5]
    for x in (g, o):
        x.setup(starts[0], goals[0], radii[0])
    g.construct_roadmap()
    o.construct_roadmap(1500)
    answers = oracle_loop(o, starts, goals, radii)
    for st, sc, gi, _ in answers:
        assert st == capi.ERR_NO_SOLUTION_FOUND and len(sc) > 0 and len(gi) > 0
    B = Batch(g, starts, goals, radii)
    assert_batch_equals_oracle(g, B, answers)
    g.close()


def test_a_roadmap_beyond_the_lds_visited_bitmap():
    """270,000 milestones: more than the 2^18 whose visited bits the search kernel keeps in LDS, so the variant without them runs;
    the reference here is set_problem + solve on the same handle (the host breadth-first search), the oracle being O(n^2)"""
    P = dict(dim=3, bounds=[(0.0, 10.0)] * 3, radius=0.19, fraction=0.05, seed=8, stream=1, max_milestones=270000,
             max_samples=10 ** 9, boxes=[([4.5, 0.0, 0.0], [5.5, 6.0, 10.0])], spheres=[([2.0, 8.0, 5.0], 1.5)])
    g = make_gpu_prm(P)
    g.setup([1.0, 1.0, 1.0], [9.0, 9.0, 9.0], 0.5)
    g.construct_roadmap()
    n, entries, _ = g.sizes()
    assert n == 270000 > (1 << 18) and entries > 4 * n
    starts, goals, radii = seeded_queries(32, 3, 0.3, 0.6)
    B = Batch(g, starts, goals, radii)
    B.check_rows_are_milestones(g.roadmap()[0])
    assert_batch_equals_single_solves(g, B, starts, goals, radii, sets_every=8)
    assert np.sum(B.status == capi.OK) >= 8 and B.len.max() > 20
    g.close()


# ------------------------------------------------------------------------------------------------ 8. translated and scaled spaces
@pytest.mark.parametrize("scale,offset", [(1.0, 1.0e3), (1.0, 1.0e6), (1.0e-12, 0.0), (1.0e18, 0.0), (1.0e60, 0.0)])
def test_translated_and_scaled_spaces(scale, offset):
    """the scenes of test_prm_translated_and_scaled_spaces; one start far outside the bounds (the per-query filter margin)"""
    dim = 3
    rng = np.random.default_rng(5)
    centres = rng.uniform(1.0, 9.0, size=(12, dim)) * scale + offset
    sph_r = rng.uniform(0.3, 0.9, size=12) * scale
    lo, hi = 0.0 * scale + offset, 10.0 * scale + offset
    P = dict(dim=dim, bounds=[(lo, hi)] * dim, radius=1.3 * scale, fraction=0.05, seed=123, stream=9,
             max_milestones=1500, max_samples=10 ** 9, boxes=[],
             spheres=[(list(map(float, c)), float(r)) for c, r in zip(centres, sph_r)])
    g, o = make_gpu_prm(P), make_oracle_prm(P)
    s, gc = [0.4 * scale + offset] * dim, [9.6 * scale + offset] * dim
    for x in (g, o):
        x.setup(s, gc, 1.0 * scale)
    g.construct_roadmap()
    o.construct_roadmap(1500)
    q = np.random.default_rng(SEED)
    starts = q.uniform(0.0, 10.0, size=(32, dim)) * scale + offset
    goals = q.uniform(0.0, 10.0, size=(32, dim)) * scale + offset
    radii = q.uniform(0.8, 1.6, size=32) * scale
    starts[5] = (1.0e4 * scale + offset) * np.array([1.0, -1.0, 1.0])     # far outside the bounds
    starts[9] = g.roadmap()[0][3] + 1.0e3 * scale * np.array([1.0, 0.0, 0.0])
    answers = oracle_loop(o, starts, goals, radii)
    assert mix(answers)[0] >= 8
    B = Batch(g, starts, goals, radii)
    assert_batch_equals_oracle(g, B, answers)
    assert_batch_equals_single_solves(g, B, starts, goals, radii, sets_every=4)
    g.close()


# ------------------------------------------------------------------------------------------------ 9. non-interference
def test_a_batch_leaves_the_handle_as_it_was(r6_4096):
    g, starts, goals, radii, answers = r6_4096
    g.set_problem([2.0] * 6, [8.0] * 6, 2.5)
    st0, path0 = g.solve()
    sc0, gi0 = (a.copy() for a in g.query_sets())
    n0 = g.sizes()
    Batch(g, starts, goals, radii)
    sc1, gi1 = g.query_sets()                                  # the last solve's sets, not the batch's
    assert np.array_equal(sc0, sc1) and np.array_equal(gi0, gi1)
    st1, path1 = g.solve()                                     # the handle's own problem definition
    assert st1 == st0 and np.array_equal(bits(path0), bits(path1))
    assert g.sizes() == n0


def test_setup_drops_the_batch_and_construction_is_unchanged():
    P = _r6_params(1024, 3.5)
    g = make_gpu_prm(P)
    g.setup([2.0] * 6, [8.0] * 6, 2.5)
    g.construct_roadmap()
    before = g.roadmap()
    starts, goals, radii = seeded_queries(64, 6, 1.5, 2.5)
    ref = Batch(g, starts, goals, radii)
    g.setup([2.0] * 6, [8.0] * 6, 2.5)                         # clears the roadmap: the batch's results go with it
    for call in (g.batch_results, g.batch_paths, lambda: g.batch_query_sets(0)):
        with pytest.raises(capi.OxhipError) as ei:
            call()
        assert ei.value.status == capi.ERR_UNSAMPLED_STATE_SPACE
    g.construct_roadmap()
    after = g.roadmap()
    assert np.array_equal(bits(before[0]), bits(after[0])) and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
    Batch(g, starts, goals, radii).same_as(ref)
    g.close()


# ------------------------------------------------------------------------------------------------ 10. SO(3) and the Python surface
def test_so3_fixture_64_queries_against_the_python_checker():
    sc = gp3.scenes()["fixture"]
    cones = g3.Cones(sc["cones"])
    rm = gp3.prm_construct(sc["bounds"], sc["radius"], sc["fraction"], cones, sc["seed"], sc["stream"], sc["max_milestones"], sc["max_samples"])
    rng = np.random.default_rng(SEED)
    qs = list(sc["queries"])
    for _ in range(60):
        s = g3.normalise([float(v) for v in rng.standard_normal(4)])
        t = g3.normalise([float(v) for v in rng.standard_normal(4)])
        qs.append((s, t, float(rng.uniform(0.2, 0.6))))
    g = make_so3_prm(sc)
    g.setup(*qs[0])
    g.construct_roadmap()
    assert g.sizes()[0] == 500
    starts, goals, radii = [q[0] for q in qs], [q[1] for q in qs], [q[2] for q in qs]
    B = Batch(g, starts, goals, radii)
    B.check_rows_are_milestones(g.roadmap()[0])
    solved = 0
    for k, (s, t, r) in enumerate(qs):
        status, s_conn, g_idx, path = gp3.prm_solve(sc["radius"], sc["fraction"], cones, rm, s, t, r)
        assert STATUS_NAME[int(B.status[k])] == status, k
        want = np.array(path, dtype=np.float64).reshape(-1, 4)
        assert want.shape == B.path(k).shape and np.array_equal(bits(want), bits(B.path(k))), k
        bsc, bgi = g.batch_query_sets(k)
        assert list(bsc) == s_conn and list(bgi) == g_idx, k
        solved += status == "solved"
    assert 16 <= solved < 64                                   # (by the checker: both outcomes occur)
    g.close()


def test_python_surface_solve_batch_on_the_wall_scene():
    from oxmpl_amd.base import ProblemDefinition, RealVectorState, RealVectorStateSpace, SphereBoxValidityChecker
    from oxmpl_amd.geometric import PRM, _MESSAGES

    class Goal:
        def __init__(self, target, radius):
            self.target, self.radius = target, radius

    P = _golden("prm_golden.json")["wall"]["params"]
    space = RealVectorStateSpace(2, [tuple(b) for b in P["bounds"]])

    def problem(start, goal, r):
        return ProblemDefinition(space, RealVectorState(start), Goal(RealVectorState(goal), r))

    planner = PRM(5.0, 0.5, problem([1.0, 5.0], [9.0, 5.0], 0.5), max_milestones=1500, seed=3)
    planner.setup(SphereBoxValidityChecker(boxes=[(lo, hi) for lo, hi in P["boxes"]]))
    planner.construct_roadmap()
    pds = [problem([1.0, 5.0], [9.0, 5.0], 0.5), problem([5.0, 5.0], [9.0, 5.0], 0.5), problem([1.0, 5.0], [20.0, 20.0], 0.5),
           problem([9.0, 9.0], [1.0, 1.0], 0.4)]
    out = planner.solve_batch(pds, 5.0)
    assert len(out) == 4
    lo, hi = params_boxes(P)

    def valid(p):
        return not any(all(lo[b][k] <= p[k] <= hi[b][k] for k in range(2)) for b in range(len(lo)))

    for k in (0, 3):
        rows = [s.values for s in out[k].states]
        assert isinstance(out[k].states[0], RealVectorState) and len(rows) >= 2
        assert orc.distance(rows[0], pds[k].start_state.values) < 1e-9
        assert orc.distance(rows[-1], pds[k].goal.target.values) <= pds[k].goal.radius
        assert is_path_valid(rows, [tuple(b) for b in P["bounds"]], P["fraction"], valid, orc.maximum_extent, orc.num_steps,
                             orc.interpolate, orc.distance)
        planner.set_problem_definition(pds[k])
        assert np.array_equal(bits([s.values for s in planner.solve(5.0).states]), bits(rows))
    assert isinstance(out[1], Exception) and str(out[1]) == _MESSAGES[capi.ERR_INVALID_START_STATE]
    assert isinstance(out[2], Exception) and str(out[2]) == _MESSAGES[capi.ERR_NO_SOLUTION_FOUND]


def test_python_surface_solve_batch_on_so3():
    from oxmpl_amd.base import ProblemDefinition, SO3ConeValidityChecker, SO3State, SO3StateSpace
    from oxmpl_amd.geometric import PRM, _MESSAGES

    class Goal:
        def __init__(self, target, radius):
            self.target, self.radius = target, radius

    start = g3.quaternion_from_axis_angle([0.0, 1.0, 0.0], g3.PI / 2.0)
    target = g3.quaternion_from_axis_angle([0.0, 1.0, 0.0], -g3.PI / 2.0)
    goal_r = 10.0 * (g3.PI / 180.0)
    cone = ([0.0, 0.0, 0.0, 1.0], 44.9 * (g3.PI / 180.0))

    def problem(s, t, r):
        return ProblemDefinition.from_so3(SO3StateSpace(), SO3State(*s), Goal(SO3State(*t), r))

    planner = PRM(5.0, 0.5, problem(start, target, goal_r), max_milestones=2000, seed=1)
    planner.setup(SO3ConeValidityChecker([(SO3State(*cone[0]), cone[1])]))
    planner.construct_roadmap()
    pds = [problem(start, target, goal_r), problem(target, start, goal_r), problem(cone[0], target, goal_r)]
    out = planner.solve_batch(pds, 5.0)
    for k, (s, t) in enumerate(((start, target), (target, start))):
        rows = [x.values for x in out[k].states]
        assert isinstance(out[k].states[0], SO3State) and len(rows) >= 2
        assert g3.distance(rows[0], s) < 1e-9 and g3.distance(rows[-1], t) <= goal_r
        assert g3.is_so3_path_valid(rows, g3.Cones([cone]), 0.05)
    assert isinstance(out[2], Exception) and str(out[2]) == _MESSAGES[capi.ERR_INVALID_START_STATE]
    with pytest.raises(ValueError):
        from oxmpl_amd.base import RealVectorState, RealVectorStateSpace
        planner.solve_batch([ProblemDefinition(RealVectorStateSpace(2, [(0.0, 1.0)] * 2), RealVectorState([0.1, 0.1]),
                                               Goal(RealVectorState([0.9, 0.9]), 0.1))], 5.0)


# ------------------------------------------------------------------------------------------------ 11. timeout
def test_timeout_leaves_a_suffix_unanswered(r6_4096):
    g, starts, goals, radii, answers = r6_4096
    ref = Batch(g, starts, goals, radii)
    for timeout in (2e-6, 2e-4, 5e-3, 3600.0):
        B = Batch(g, starts, goals, radii, timeout_s=timeout, chunk_queries=1)
        timed_out = B.status == capi.ERR_TIMEOUT
        first = int(np.argmax(timed_out)) if timed_out.any() else 256
        print("timeout %g s: %d of 256 queries answered" % (timeout, first))
        assert first >= 1 and np.all(timed_out[first:]) and not timed_out[:first].any()      # a suffix; the first round always runs
        assert B.timing["rounds"] == first
        assert np.all(B.len[first:] == 0)
        for a, b in ((B.status, ref.status), (B.len, ref.len), (B.goal, ref.goal), (B.ns, ref.ns), (B.ng, ref.ng)):
            assert np.array_equal(a[:first], b[:first])
        n_rows = int(ref.off[first])
        assert np.array_equal(B.nodes, ref.nodes[:n_rows]) and np.array_equal(bits(B.rows), bits(ref.rows[:n_rows]))
    assert first == 256                                        # an hour is enough
