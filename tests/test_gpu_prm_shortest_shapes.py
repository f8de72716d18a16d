"""GPU: the shortest-path PRM batch (prm_shortest.hip) on the scenes of tests/prm_shortest_shapes.py -- ties
under distance weights, deep levels, every lane group, every dimension, isolated milestones -- and at its boundaries: one
milestone, the label-round cap reached exactly, more queries than one round takes.  The reference is the pure-Python checker
(tests/golden/make_golden_prm_shortest.py) on the device's own roadmap and query sets; every comparison is bit for bit.
tests/test_prm_shortest_shapes_model.py shows on the CPU that the scenes hold what they are here for."""
import numpy as np
import pytest

from helpers import bits
import prm_shortest_shapes as shapes
from prm_shortest_shapes import gsp, mg

pytestmark = pytest.mark.gpu

from oxmpl_amd import capi  # noqa: E402
from prm_shortest_helpers import Batch, RoadmapChecker, make_gpu_prm, DISTANCE, UNIT, ZERO  # noqa: E402

NAMES = sorted(shapes.SCENES)
MAX_ROUND = 65535                                              # queries per round at the most (solve_batch_common)


class ShapeScene(RoadmapChecker):
    """a scene's roadmap on the device, its queries, and the four batches that answer them"""

    def __init__(self, name, n_queries=None, batches=True, **kw):
        self.name, self.dist = name, mg.distance
        self.starts, self.goals, self.radii = shapes.queries(name, n_queries)
        self.g = make_gpu_prm(shapes.SCENES[name], **kw)
        self.g.setup(self.starts[0], self.goals[0], self.radii[0])
        self.g.construct_roadmap()
        self.load_roadmap()
        self._sets, self._res, self.B, self.rounds = {}, {}, {}, {}
        if batches:
            self.bfs = self.batch(None)
            for mode in (UNIT, ZERO, DISTANCE):
                self.B[mode] = self.batch(mode)
                self.rounds[mode] = self.g.batch_search_stats()["label_rounds"].copy()

    def batch(self, mode, **kw):
        return Batch(self.g, self.starts, self.goals, self.radii, weights=mode, **kw)

    def checker(self, B, q, mode):
        """Unlike RoadmapChecker.checker, kept per (mode, query): the query sets are those of the first batch that asked, and
        every later batch of the same queries (chunked, another mode) is held to them.  The batch must hold the scene's own
        queries in their own order."""
        assert np.array_equal(bits(B.starts[q]), bits(np.array(self.starts[q])))
        if q not in self._sets:
            self._sets[q] = tuple([int(v) for v in a] for a in self.g.batch_query_sets(q))
        if (mode, q) not in self._res:
            sc, gi = self._sets[q]
            init = gsp.init_labels(self.n, sc, self.starts[q], self.states, self.dist, mode)
            self._res[(mode, q)] = gsp.shortest_query(self.edges, self.weights(mode), init, gi)
        return self._res[(mode, q)]


_scenes = {}


def _get(name):
    if name not in _scenes:
        _scenes[name] = ShapeScene(name)
    return _scenes[name]


@pytest.fixture(scope="module", params=NAMES)
def shape(request):
    return _get(request.param)


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for s in _scenes.values():
        s.g.close()
    _scenes.clear()


# ------------------------------------------------------------------------------------------------ 1. the scenes
def test_the_roadmap_selects_the_group_the_model_found(shape):
    s = shape
    n, entries, _ = s.g.sizes()
    assert n == s.n == shapes.SCENES[s.name]["max_milestones"] and entries == sum(len(lst) for lst in s.edges)
    assert shapes.library_group(n, entries) == shapes.batch_group(n, entries) == shapes.GROUP[s.name]
    assert set(shapes.GROUP.values()) == {4, 8, 16, 32, 64}


def test_the_library_s_group_is_the_transcription_s_at_its_thresholds():
    for n, entries in ((1, 0), (10, 40), (10, 41), (10, 80), (10, 81), (10, 160), (10, 161), (10, 320), (10, 321), (10, 6400)):
        assert shapes.library_group(n, entries) == shapes.batch_group(n, entries)


def test_distance_and_unit_batches_equal_the_checker(shape):
    s = shape
    q = shapes.n_queries(s.name)
    for mode in (DISTANCE, UNIT):
        B = s.B[mode]
        assert len(B.status) == q
        B.check_rows_are_milestones(s.states)
        solved = s.check_against_checker(B, mode)
        assert s.compared == q                                     # no obstacles: no query is left out
        assert solved == int(np.sum(B.status == capi.OK))
    if s.name == "dust":
        assert solved == 0
    else:
        assert solved >= (2 if s.name == "sparse" else q // 2)


def test_zero_weights_give_the_unit_node_lists(shape):
    U, Z = shape.B[UNIT], shape.B[ZERO]
    for a, b in ((U.status, Z.status), (U.nodes, Z.nodes), (U.off, Z.off), (U.goal, Z.goal), (bits(U.rows), bits(Z.rows))):
        assert np.array_equal(a, b)
    ok = U.status == capi.OK
    assert np.all(Z.cost[ok] == 0.0) and np.array_equal(U.cost[ok], U.len[ok].astype(np.float64) - 1.0)


def test_statuses_sets_and_unit_lengths_are_the_bfs_batch_s(shape):
    s = shape
    for mode in (DISTANCE, UNIT, ZERO):
        for a, b in ((s.B[mode].status, s.bfs.status), (s.B[mode].ns, s.bfs.ns), (s.B[mode].ng, s.bfs.ng)):
            assert np.array_equal(a, b)
    assert np.array_equal(s.B[UNIT].len, s.bfs.len) and np.all(s.B[DISTANCE].len >= s.bfs.len)
    assert not np.any(s.bfs.status == capi.ERR_INVALID_START_STATE)


def test_the_path_s_left_to_right_cost_is_its_label(shape):
    s = shape
    B = s.B[DISTANCE]
    for q in np.nonzero(B.status == capi.OK)[0]:
        assert bits(np.float64(gsp.path_cost(B.starts[q], B.path_nodes(q)[1:], s.states, s.dist))) == bits(np.float64(B.cost[q])), q


def test_label_rounds_stay_within_their_cap(shape):
    s = shape
    for mode in (DISTANCE, UNIT, ZERO):
        rounds, ns = s.rounds[mode], s.B[mode].ns
        assert len(rounds) == len(ns)
        assert np.all(rounds <= s.n) and np.all(rounds[ns > 0] >= 1) and np.all(rounds[ns == 0] == 0)


# ------------------------------------------------------------------------------------------------ 2. every label
def _deepest(s, mode):
    """(query, hops) of the deepest tight levels among the scene's queries, by the checker"""
    depth = [max((h for h in s.checker(s.B[mode], q, mode)["hops"] if h != gsp.UNSET), default=0) for q in range(len(s.radii))]
    return int(np.argmax(depth)), max(depth)


@pytest.mark.parametrize("name", shapes.ALL_LABELS)
def test_all_labels_hops_and_parents(name):
    s = _get(name)
    for mode in (DISTANCE, UNIT):
        B = s.batch(mode)                                          # batch_labels answers for the last batch
        solved = [int(q) for q in np.nonzero(B.status == capi.OK)[0]]
        dry = [int(q) for q in np.nonzero(B.status == capi.ERR_NO_SOLUTION_FOUND)[0]]
        deep_q, deep = _deepest(s, mode)
        for q in solved[:2] + solved[-1:] + dry[:1] + [deep_q]:
            res = s.checker(B, q, mode)
            cost, hops, parent = s.g.batch_labels(q)
            assert np.array_equal(bits(cost), bits(np.array(res["c"], dtype=np.float64))), (mode, q)
            assert [int(v) for v in hops] == res["hops"] and [int(v) for v in parent] == res["parent"], (mode, q)
            assert np.array_equal(np.isinf(cost), hops == gsp.UNSET)
        hops = s.g.batch_labels(deep_q)[1]
        assert int(hops[hops != gsp.UNSET].max()) == deep
        if mode == DISTANCE and name in ("line", "strip"):
            assert deep >= 40


def test_distance_weights_meet_the_tie_rule_on_the_line_and_not_on_the_strip():
    """What the model test pins, counted again on the device's roadmap and query sets: nodes with two or more tight predecessors
    one level up, and answers whose chain passes through one."""
    count = {}
    for name in ("line", "line_dense", "strip"):
        s = _get(name)
        count[name] = chains = 0
        for q in range(len(s.radii)):
            res = s.checker(s.B[DISTANCE], q, DISTANCE)
            cnt = shapes.multi_tight(s.edges, s.weights(DISTANCE), res)
            count[name] += sum(k >= 2 for k in cnt)
            chains += res["status"] == "solved" and any(cnt[v] >= 2 for v in res["nodes"])
        if name == "line":
            assert chains >= 1
    assert count["line"] >= 1000 and count["line_dense"] >= 1000 and count["strip"] == 0


# ------------------------------------------------------------------------------------------------ 3. chunking on the line
def test_the_line_s_answers_do_not_depend_on_chunking_or_order():
    s = _get("line")
    ref = s.B[DISTANCE]
    q = len(s.radii)
    assert ref.timing["rounds"] == 1
    for chunk, rounds in ((1, q), (7, (q + 6) // 7)):
        B = s.batch(DISTANCE, chunk_queries=chunk)
        assert B.timing["rounds"] == rounds
        B.same_as(ref)
    rev = Batch(s.g, s.starts[::-1], s.goals[::-1], s.radii[::-1])
    for a, b in ((rev.status, ref.status), (rev.len, ref.len), (rev.goal, ref.goal), (rev.ns, ref.ns), (rev.ng, ref.ng), (bits(rev.cost), bits(ref.cost))):
        assert np.array_equal(a[::-1], b)
    for k in range(q):
        assert rev.path_nodes(q - 1 - k) == ref.path_nodes(k) and np.array_equal(bits(rev.path(q - 1 - k)), bits(ref.path(k)))


# ------------------------------------------------------------------------------------------------ 4. one and two milestones
class Tiny(RoadmapChecker):
    """the first `n` milestones of the [0, 10]^2 scenes' stream, connected within `radius`"""

    def __init__(self, n, radius):
        self.dist = mg.distance
        self.g = make_gpu_prm(dict(shapes.SCENES["g8"], max_milestones=n, radius=radius))
        self.g.setup([5.0, 5.0], [5.0, 5.0], 1.0)
        self.g.construct_roadmap()
        self.load_roadmap()
        assert self.n == n


def _labels_equal_the_checker(s, B, mode):
    for q in range(len(B.status)):
        res = s.checker(B, q, mode)
        cost, hops, parent = s.g.batch_labels(q)
        assert np.array_equal(bits(cost), bits(np.array(res["c"], dtype=np.float64))), (mode, q)
        assert [int(v) for v in hops] == res["hops"] and [int(v) for v in parent] == res["parent"], (mode, q)


def test_one_milestone():
    """n = 1: no edge entries, so no weights are computed and the kernels get a null weights array; the only label round is the
    cap."""
    s = Tiny(1, 4.0)
    try:
        assert s.g.sizes()[:2] == (1, 0) and s.edges == [[]]
        m = [float(v) for v in s.states[0]]
        near = [m[0] + (0.5 if m[0] < 5.0 else -0.5), m[1]]
        far = [9.75 if m[0] < 5.0 else 0.25, 9.75 if m[1] < 5.0 else 0.25]
        assert mg.distance(near, m) < 4.0 < mg.distance(far, m)
        starts, goals, radii = [near, near, far], [m, far, m], [0.25, 0.25, 0.25]
        bfs = Batch(s.g, starts, goals, radii, weights=None)
        for mode, d in ((DISTANCE, mg.distance(near, m)), (UNIT, 1.0), (ZERO, 0.0)):
            B = Batch(s.g, starts, goals, radii, weights=mode)
            assert [int(v) for v in B.status] == [capi.OK, capi.ERR_NO_SOLUTION_FOUND, capi.ERR_NO_SOLUTION_FOUND]
            assert [int(v) for v in B.ns] == [1, 1, 0] and [int(v) for v in B.ng] == [1, 0, 1]
            assert [int(v) for v in B.len] == [2, 0, 0] and int(B.goal[0]) == 0 and B.path_nodes(0)[1:] == [0]
            assert bits(np.float64(B.cost[0])) == bits(np.float64(d))
            assert [int(v) for v in s.g.batch_search_stats()["label_rounds"]] == [1, 1, 0]      # 1 == n: the cap, reached and not hit
            assert B.timing["rounds"] == 1
            B.check_rows_are_milestones(s.states)
            for a, b in ((B.status, bfs.status), (B.ns, bfs.ns), (B.ng, bfs.ng), (B.len, bfs.len)):
                assert np.array_equal(a, b)
            assert s.check_against_checker(B, mode) == 1 and s.compared == 3
            _labels_equal_the_checker(s, B, mode)
            for q, (c, h, p) in enumerate(((d, 0, gsp.ROOT), (d, 0, gsp.ROOT), (gsp.INF, gsp.UNSET, gsp.UNSET))):
                cost, hops, parent = s.g.batch_labels(q)
                assert bits(cost)[0] == bits(np.float64(c)) and (int(hops[0]), int(parent[0])) == (h, p), (mode, q)
    finally:
        s.g.close()


def test_two_milestones_reach_the_label_round_cap_exactly():
    """A chain of two whose start connects to one end: the second label round settles the far end, and rounds == n == 2 is an
    answer, not the cap's error."""
    probe = Tiny(2, 1.0)
    m0, m1 = ([float(v) for v in row] for row in probe.states)
    probe.g.close()
    d = mg.distance(m0, m1)
    assert d > 0.0
    s = Tiny(2, 1.5 * d)
    try:
        assert np.array_equal(bits(s.states), bits(np.array([m0, m1]))) and s.edges == [[1], [0]]
        beyond0 = [a + 0.75 * (a - b) for a, b in zip(m0, m1)]
        beyond1 = [b + 0.75 * (b - a) for a, b in zip(m0, m1)]
        assert mg.distance(beyond0, m0) < 1.5 * d < mg.distance(beyond0, m1)
        assert mg.distance(beyond1, m1) < 1.5 * d < mg.distance(beyond1, m0)
        starts, goals, radii = [beyond0, beyond1], [m1, m0], [0.25 * d, 0.25 * d]
        w = mg.distance(m0, m1)
        want = {DISTANCE: [mg.distance(beyond0, m0) + w, mg.distance(beyond1, m1) + w], UNIT: [2.0, 2.0], ZERO: [0.0, 0.0]}
        for mode in (DISTANCE, UNIT, ZERO):
            B = Batch(s.g, starts, goals, radii, weights=mode)
            assert [int(v) for v in B.status] == [capi.OK, capi.OK]
            assert [int(v) for v in B.ns] == [1, 1] and [int(v) for v in B.ng] == [1, 1]
            assert B.path_nodes(0)[1:] == [0, 1] and B.path_nodes(1)[1:] == [1, 0]
            assert np.array_equal(bits(B.cost), bits(np.array(want[mode])))
            assert [int(v) for v in s.g.batch_search_stats()["label_rounds"]] == [2, 2]
            B.check_rows_are_milestones(s.states)
            assert s.check_against_checker(B, mode) == 2 and s.compared == 2
            _labels_equal_the_checker(s, B, mode)
            cost, hops, parent = s.g.batch_labels(0)
            assert [int(v) for v in hops] == [0, 1] and [int(v) for v in parent] == [gsp.ROOT, 0]
            cost, hops, parent = s.g.batch_labels(1)
            assert [int(v) for v in hops] == [1, 0] and [int(v) for v in parent] == [1, gsp.ROOT]
    finally:
        s.g.close()


# ------------------------------------------------------------------------------------------------ 5. more queries than one round takes
def test_more_queries_than_one_round_takes():
    """65,600 queries on the first 64 milestones of the line: the automatic chunk stops at 65,535, so the call takes two rounds, and
    the second round's few queries land where the first round's left off."""
    Q = MAX_ROUND + 65
    s = ShapeScene("line", n_queries=Q, batches=False, max_milestones=64)
    try:
        assert s.n == 64 and len(s.radii) == Q
        auto = s.batch(DISTANCE, chunk_queries=0)
        assert auto.timing["rounds"] == 2
        rounds_auto = s.g.batch_search_stats()["label_rounds"].copy()
        solved = np.nonzero(auto.status == capi.OK)[0]
        assert len(solved) >= 30 and not np.any(auto.status == capi.ERR_INVALID_START_STATE)
        sample = {MAX_ROUND - 1, MAX_ROUND, MAX_ROUND + 1}
        sample.update(int(q) for q in solved[::len(solved) // 30][:30])
        rng = np.random.default_rng(shapes.QUERY_SEED)
        while len(sample) < 64:
            sample.add(int(rng.integers(0, Q)))
        sample = sorted(sample)
        assert s.check_against_checker(auto, DISTANCE, sample) >= 30 and s.compared == 64
        auto.check_rows_are_milestones(s.states)
        assert np.all(rounds_auto <= s.n) and np.all(rounds_auto[auto.ns > 0] >= 1)
        nine = s.batch(DISTANCE, chunk_queries=8192)
        assert nine.timing["rounds"] == 9
        nine.same_as(auto)
        bfs = s.batch(None, chunk_queries=0)
        assert bfs.timing["rounds"] == 2
        for a, b in ((bfs.status, auto.status), (bfs.ns, auto.ns), (bfs.ng, auto.ng)):
            assert np.array_equal(a, b)
        bfs9 = s.batch(None, chunk_queries=8192)
        assert bfs9.timing["rounds"] == 9
        bfs9.same_as(bfs)
    finally:
        s.g.close()
