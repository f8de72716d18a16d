"""GPU: a roadmap planted from the host (oxhip_prm_set_roadmap) and a roadmap re-checked against the scene as it is now
(oxhip_prm_revalidate), DESIGN.md section 20.  Every comparison is bit for bit.  The references: the handle that built the roadmap
(round trips), tests/golden/prm_revalidate.json (pure Python), and -- independently of any fixture -- the plain filter computed
from oxhip_rrt_batch_is_valid / oxhip_rrt_batch_check_motion on an RRT batch of the same space, bounds, fraction and obstacles,
the motion taken from the higher index to the lower.

Direction: the fixture's generator found a pair (a, b), both valid, with check_motion(a -> b) invalid and check_motion(b -> a) valid
(after 70 grazing pairs); it is planted both ways round and each verdict asserted."""
import math

import numpy as np
import pytest

from helpers import bits, params_boxes, params_spheres, unhex
from prm_helpers import csr_checksum, states_checksum
from prm_revalidate_helpers import added_spheres, csr, edge_lists, fixture, plain_filter, unhex_rows, valid_mask

pytestmark = pytest.mark.gpu

from oxmpl_amd import capi  # noqa: E402

SCENES = ["r2_radius", "r6_knn", "so3"]
CHANGED = SCENES + ["r2_small"]   # (the small scene's filtered CSR is in the fixture in full)
SO3_UNBOUNDED = [0.0, 0.0, 0.0, 1.0, math.pi]
R2 = dict(dim=2, bounds=[(0.0, 10.0), (0.0, 10.0)], radius=1.0, fraction=0.05)


# ---------------------------------------------------------------------------------------------------------------- scenes
def _obstacles(name, added):
    """(sphere / cone centres, radii, box lo, box hi) of a fixture scene, with the added obstacles on top when asked"""
    sc = fixture()[name]
    P = sc["params"]
    if name == "so3":
        c = unhex_rows([cc for cc, _ in P["cones"]])
        r = np.array([unhex(rr) for _, rr in P["cones"]])
        lo = hi = np.zeros((0, 4))
    else:
        c, r = params_spheres(P)
        lo, hi = params_boxes(P)
    if added:
        ac, ar = added_spheres(sc)
        c, r = np.vstack([c.reshape(-1, ac.shape[1]), ac]), np.concatenate([r, ar])
        if name != "so3" and sc["added"]["boxes"]:
            lo = np.vstack([lo, [b[0] for b in sc["added"]["boxes"]]])
            hi = np.vstack([hi, [b[1] for b in sc["added"]["boxes"]]])
    return c, r, lo, hi


def _set_obstacles(g, name, added):
    c, r, lo, hi = _obstacles(name, added)
    if len(r):
        g.set_spheres(c, r)
    if len(lo):
        g.set_boxes(lo, hi)


def scene_prm(name, added=False):
    P = fixture()[name]["params"]
    if name == "so3":
        g = capi.PRMRoadmap(4, SO3_UNBOUNDED, unhex(P["radius"]), P["max_milestones"], lvs_fraction=unhex(P["fraction"]),
                            seed=P["seed"], stream=P["stream"], space=capi.SPACE_SO3)
    else:
        g = capi.PRMRoadmap(P["dim"], P["bounds"], P["radius"], P["max_milestones"], lvs_fraction=P["fraction"], seed=P["seed"],
                            stream=P["stream"], knn_k=P.get("knn_k", 0))
    _set_obstacles(g, name, added)
    return g


def scene_rrt(name, added=True):
    """an RRT batch of the scene's space, bounds, fraction and obstacles: the independent is_valid / check_motion"""
    P = fixture()[name]["params"]
    if name == "so3":
        b = capi.RRTBatch(4, SO3_UNBOUNDED, 0.5, 0.05, 1, max_nodes=64, lvs_fraction=unhex(P["fraction"]), space=capi.SPACE_SO3)
    else:
        b = capi.RRTBatch(P["dim"], P["bounds"], 1.0, 0.05, 1, max_nodes=64, lvs_fraction=P["fraction"])
    _set_obstacles(b, name, added)
    return b


def scene_queries(name, q=64):
    rng = np.random.default_rng(20261019 + CHANGED.index(name))
    if name == "so3":
        s, g = rng.normal(size=(q, 4)), rng.normal(size=(q, 4))
        return s / np.linalg.norm(s, axis=1)[:, None], g / np.linalg.norm(g, axis=1)[:, None], np.full(q, 0.35)
    dim = fixture()[name]["params"]["dim"]
    return rng.uniform(0.2, 9.8, size=(q, dim)), rng.uniform(0.2, 9.8, size=(q, dim)), np.full(q, 1.0 if dim == 2 else 3.5)


def setup_any(g):
    if g.space == capi.SPACE_SO3:
        g.setup([0.0, 1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], 0.2)
    else:
        g.setup([0.5] * g.dim, [9.5] * g.dim, 0.5)


def answers(g, queries):
    """what solve_batch and solve_batch_shortest return for the queries, as comparable arrays"""
    s, t, r = queries
    out = []
    for shortest in (False, True):
        st = (g.solve_batch_shortest if shortest else g.solve_batch)(s, t, r).copy()
        res = g.batch_results()
        off, nodes, rows = g.batch_paths()
        out += [st, res["path_len"], res["goal_node"], res["n_start"], res["n_goal"], off, nodes, bits(rows)]
        if shortest:
            out.append(bits(g.batch_costs()))
    return out


def assert_same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def assert_roadmap_equal(a, b):
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


_BUILT = {}


def built(name):
    """the scene's roadmap as the device constructs it in the scene BEFORE the obstacles were added (once per module)"""
    if name not in _BUILT:
        g = scene_prm(name)
        setup_any(g)
        g.construct_roadmap()
        _BUILT[name] = (g, g.roadmap())
    return _BUILT[name]


def planted(name, roadmap, added):
    g = scene_prm(name, added)
    setup_any(g)
    g.set_roadmap(*roadmap)
    return g


def independent_filter(rrt, states, lists):
    """(valid, filtered lists) from the RRT batch's own is_valid / check_motion, from = the higher index"""
    valid = rrt.is_valid(states)
    pairs = [(j, i) for j, row in enumerate(lists) for i in row if i < j and valid[i] and valid[j]]
    ok = {}
    if pairs:
        idx = np.array(pairs)
        ok = dict(zip(pairs, rrt.check_motion(states[idx[:, 0]], states[idx[:, 1]])))
    return valid, plain_filter(lists, valid, ok)


# ---------------------------------------------------------------------------------------------------------------- round trip
@pytest.mark.parametrize("name", SCENES)
def test_round_trip_is_bit_identical_and_answers_alike(name):
    sc = fixture()[name]
    g0, rm = built(name)
    assert len(rm[0]) == sc["n"] and "%016x" % states_checksum(rm[0]) == sc["states_checksum"]       # the fixture's roadmap
    assert "%016x" % csr_checksum(rm[1], rm[2]) == sc["csr_checksum_before"]
    g1 = planted(name, rm, added=False)
    assert_roadmap_equal(g1.roadmap(), rm)
    assert g1.sizes() == (sc["n"], len(rm[2]), 0)                                                    # n_samples = 0
    g1.construct_roadmap()                                                                           # a no-op on a planted roadmap
    assert_roadmap_equal(g1.roadmap(), rm)
    q = scene_queries(name)
    a0 = answers(g0, q)
    assert_same(a0, answers(g1, q))
    assert np.count_nonzero(a0[0] == capi.OK) >= 8
    g0.solve_batch(*q)
    g1.solve_batch(*q)
    for k in range(64):                                                                              # the single solve, host search
        for g in (g0, g1):
            g.set_problem(q[0][k], q[1][k], q[2][k])
        (s0, p0), (s1, p1) = g0.solve(), g1.solve()
        assert s0 == s1 == a0[0][k] and np.array_equal(bits(p0), bits(p1))
    setup_any(g1)                                                                                    # setup clears a planted roadmap
    assert g1.sizes()[0] == 0


# ---------------------------------------------------------------------------------------------------------------- hand-made shapes
def _circle(n, r=3.5, centre=(5.0, 5.0)):
    a = 2.0 * np.pi * np.arange(n) / max(n, 1)
    return np.stack([centre[0] + r * np.cos(a), centre[1] + r * np.sin(a)], axis=1)


def _shape(kind):
    if kind == "one":
        return np.array([[5.0, 7.0]]), [[]]
    if kind == "two":
        return np.array([[1.0, 1.0], [1.5, 1.0]]), [[1], [0]]
    if kind in ("ring_65", "ring_257"):
        n = int(kind.split("_")[1])
        lists = [sorted({(i - 1) % n, (i + 1) % n, (i + n // 2) % n, (i - n // 2) % n} - {i}) for i in range(n)]
        return _circle(n), lists
    if kind == "star_300":        # hub 0 with 300 neighbours: its row crosses 64 and 256, every mirror search runs into a row of length 1
        return np.vstack([[[5.0, 5.0]], _circle(300, 3.0)]), [list(range(1, 301))] + [[0]] * 300
    if kind == "star_hub_last":   # the same with the hub as the highest index: the hub's row is all lower entries
        return np.vstack([_circle(300, 3.0), [[5.0, 5.0]]]), [[300]] * 300 + [list(range(300))]
    assert kind == "no_edges"
    return _circle(70), [[] for _ in range(70)]


@pytest.mark.parametrize("kind", ["one", "two", "ring_65", "ring_257", "star_300", "star_hub_last", "no_edges"])
def test_hand_made_shapes_plant_and_recheck(kind):
    states, lists = _shape(kind)
    off, nb = csr(lists)
    g = capi.PRMRoadmap(2, R2["bounds"], R2["radius"], 512, lvs_fraction=R2["fraction"])
    g.setup([0.5, 0.5], [9.5, 9.5], 0.5)
    g.set_roadmap(states, off, nb)
    assert_roadmap_equal(g.roadmap(), (states, off, nb))
    valid, removed = g.revalidate()                      # no obstacle: nothing goes
    assert valid.all() and removed == 0
    assert_roadmap_equal(g.roadmap(), (states, off, nb))
    c, r = [[5.0, 7.6], [2.2, 3.9]], [0.9, 0.7]
    g.set_spheres(c, r)
    rrt = capi.RRTBatch(2, R2["bounds"], 1.0, 0.05, 1, max_nodes=64, lvs_fraction=R2["fraction"])
    rrt.set_spheres(c, r)
    want_valid, want = independent_filter(rrt, states, lists)
    valid, removed = g.revalidate()
    s2, o2, n2 = g.roadmap()
    assert np.array_equal(valid, want_valid) and edge_lists(o2, n2) == want and np.array_equal(bits(s2), bits(states))
    assert removed == len(nb) - len(n2) and g.sizes()[1] == len(n2)
    if kind in ("one", "star_300", "star_hub_last", "ring_257"):
        assert not valid.all()                           # the discs cover milestones of these shapes
    if kind.startswith("star"):
        assert 0 < len(n2) < len(nb) and np.count_nonzero(valid) > len(n2) // 2 + 1   # and a spoke between two valid ends is cut
    t = g.revalidate_last_timing()["phase_ms"]
    assert len(t) == 4 and all(v >= 0.0 for v in t)


# ---------------------------------------------------------------------------------------------------------------- refusals
def _ring12():
    return _circle(12), [sorted([(i - 1) % 12, (i + 1) % 12]) for i in range(12)]


def _broken(rule):
    states, lists = _ring12()
    lists = [list(r) for r in lists]
    off, nb = None, None
    if rule == "neighbour_range":
        lists[2][1] = 12
    elif rule == "self_loop":
        lists[4] = [3, 4, 5]
    elif rule == "unsorted":
        lists[5] = [6, 4]
    elif rule == "asymmetric":
        lists[7] = [8]                                   # 7 stays in row 6: the lowest offending row is 6
    off, nb = csr(lists)
    if rule == "offsets_start":
        off = off.copy(); off[0] = 1
    elif rule == "offsets_order":
        off = off.copy(); off[3], off[4] = off[4], off[3]
    return states, off, nb


ROWS = dict(offsets_start=0, offsets_order=3, neighbour_range=2, self_loop=4, unsorted=5, asymmetric=6)


def test_refused_roadmaps_name_rule_and_row_and_leave_the_handle_alone():
    states, lists = _ring12()
    g = capi.PRMRoadmap(2, R2["bounds"], 2.5, 16, lvs_fraction=R2["fraction"])
    rng = np.random.default_rng(5)
    q = (rng.uniform(1.0, 9.0, size=(16, 2)), rng.uniform(1.0, 9.0, size=(16, 2)), np.full(16, 1.5))
    with pytest.raises(capi.OxhipError) as e:            # no setup()
        g.set_roadmap(states, *csr(lists))
    assert e.value.status == capi.ERR_PLANNER_UNINITIALISED
    g.setup([0.5, 0.5], [9.5, 9.5], 0.5)
    g.set_roadmap(states, *csr(lists))
    before, ans = g.roadmap(), answers(g, q)             # (the last batch is the shortest-path one)
    assert np.count_nonzero(ans[0] == capi.OK) >= 4

    def untouched():
        assert_roadmap_equal(g.roadmap(), before)
        res = g.batch_results()
        assert np.array_equal(res["status"], ans[8]) and np.array_equal(bits(g.batch_costs()), ans[16])

    for rule, row in ROWS.items():
        with pytest.raises(capi.OxhipError) as e:
            g.set_roadmap(*_broken(rule))
        assert e.value.status == capi.ERR_BAD_ARG and rule in str(e.value) and str(e.value).endswith("row %d" % row), (rule, str(e.value))
        untouched()
    bad = states.copy()
    bad[3, 1] = np.inf
    for s, o, n, status in ((bad, *csr(lists), capi.ERR_BAD_ARG),
                            (_circle(17), *csr([[] for _ in range(17)]), capi.ERR_CAPACITY),                       # n > max_milestones
                            (states, np.array([0] * 12 + [1 << 32], dtype=np.uint64), csr(lists)[1], capi.ERR_CAPACITY)):
        with pytest.raises(capi.OxhipError) as e:
            g.set_roadmap(s, o, n)
        assert e.value.status == status
        untouched()
    assert_same(ans, answers(g, q))
    g.set_roadmap(np.zeros((0, 2)), [0], [])             # n = 0: an empty roadmap, and construct_roadmap builds again
    assert g.sizes()[:2] == (0, 0)
    with pytest.raises(capi.OxhipError) as e:
        g.revalidate()
    assert e.value.status == capi.ERR_UNSAMPLED_STATE_SPACE
    g.construct_roadmap()
    assert g.sizes()[0] == 16
    g2 = capi.PRMRoadmap(2, R2["bounds"], 2.5, 16, lvs_fraction=R2["fraction"])
    with pytest.raises(capi.OxhipError) as e:
        g2.revalidate()
    assert e.value.status == capi.ERR_PLANNER_UNINITIALISED


# ---------------------------------------------------------------------------------------------------------------- unchanged scene
@pytest.mark.parametrize("name", SCENES)
def test_unchanged_scene_removes_nothing(name):
    g = scene_prm(name)
    setup_any(g)
    g.construct_roadmap()
    rm = g.roadmap()
    g.solve_batch_shortest(*scene_queries(name, 8))
    valid, removed = g.revalidate()
    assert valid.all() and len(valid) == len(rm[0]) and removed == 0
    assert_roadmap_equal(g.roadmap(), rm)
    assert g.sizes()[2] > 0                              # the samples drawn are the constructed roadmap's still
    with pytest.raises(capi.OxhipError) as e:            # the last batch went with the re-check, as after setup()
        g.batch_costs()
    assert e.value.status == capi.ERR_UNSAMPLED_STATE_SPACE


# ---------------------------------------------------------------------------------------------------------------- changed scene
_CHANGED = {}


def changed(name):
    """the constructed roadmap planted in the scene WITH the added obstacles and re-checked there (once per module)"""
    if name not in _CHANGED:
        _, rm = built(name)
        g = planted(name, rm, added=True)
        g.solve_batch(*scene_queries(name, 4))
        valid, removed = g.revalidate()
        try:
            g.batch_costs()
            after_batch = capi.OK
        except capi.OxhipError as e:
            after_batch = e.status
        _CHANGED[name] = dict(g=g, rm=rm, valid=valid, removed=removed, after=g.roadmap(), after_batch=after_batch,
                              timing=g.revalidate_last_timing())
    return _CHANGED[name]


@pytest.mark.parametrize("name", CHANGED)
def test_changed_scene_equals_fixture_and_independent_filter(name):
    sc, ch = fixture()[name], changed(name)
    states, off, nb = ch["after"]
    assert np.array_equal(bits(states), bits(ch["rm"][0]))                                           # indices are stable
    assert np.array_equal(ch["valid"], valid_mask(sc)) and ch["removed"] == sc["removed_entries"] > 0
    assert len(nb) == sc["entries_after"] and "%016x" % csr_checksum(off, nb) == sc["csr_checksum_after"]
    if "edges_after" in sc:
        assert edge_lists(off, nb) == sc["edges_after"] and "%016x" % csr_checksum(ch["rm"][1], ch["rm"][2]) == sc["csr_checksum_before"]
    want_valid, want = independent_filter(scene_rrt(name), ch["rm"][0], edge_lists(ch["rm"][1], ch["rm"][2]))
    assert np.array_equal(ch["valid"], want_valid) and edge_lists(off, nb) == want
    assert ch["g"].sizes()[:2] == (sc["n"], len(nb))
    assert ch["after_batch"] == capi.ERR_UNSAMPLED_STATE_SPACE                                       # as after setup()
    assert len(ch["timing"]["phase_ms"]) == 4 and all(v >= 0.0 for v in ch["timing"]["phase_ms"])


@pytest.mark.parametrize("name", SCENES)
def test_answers_after_revalidation(name):
    ch = changed(name)
    g, q = ch["g"], scene_queries(name)
    fresh = planted(name, ch["after"], added=True)       # a fresh handle planted with the filtered CSR
    a = answers(g, q)
    assert_same(a, answers(fresh, q))
    assert np.count_nonzero(a[0] == capi.OK) >= 4
    rrt, states = scene_rrt(name), ch["after"][0]
    for base in (0, 8):                                  # breadth-first paths, shortest paths
        off, nodes, rows = a[base + 5], a[base + 6], a[base + 7].view(np.float64)
        frm, to = [], []
        for k in range(len(q[2])):
            lo, hi = int(off[k]), int(off[k + 1])
            assert all(ch["valid"][v] for v in nodes[lo + 1:hi])
            for e in range(lo, hi - 1):
                u, v = (None, int(nodes[e + 1])) if e == lo else (int(nodes[e]), int(nodes[e + 1]))
                if u is None:
                    frm.append(rows[e]); to.append(rows[e + 1])              # start -> first milestone
                else:
                    frm.append(states[max(u, v)]); to.append(states[min(u, v)])   # as the roadmap checked it
        assert len(frm) > 0 and rrt.check_motion(np.array(frm), np.array(to)).all()
    g.solve_batch(*q)
    g.set_problem(q[0][0], q[1][0], q[2][0])             # the single solve searches a host copy: it must be the new one
    st, path = g.solve()
    assert st == a[0][0] and np.array_equal(bits(path), a[7][int(a[5][0]):int(a[5][1])])


# ---------------------------------------------------------------------------------------------------------------- edge cases
def test_one_sphere_over_every_milestone():
    states, lists = _circle(65, 1.0), [sorted({(i - 1) % 65, (i + 1) % 65}) for i in range(65)]
    g = capi.PRMRoadmap(2, R2["bounds"], 1.0, 128, lvs_fraction=R2["fraction"])
    g.setup([0.5, 0.5], [9.5, 9.5], 0.5)
    g.set_roadmap(states, *csr(lists))
    g.set_spheres([[5.0, 5.0]], [2.0])
    valid, removed = g.revalidate()
    s, off, nb = g.roadmap()
    assert not valid.any() and removed == 130 and len(nb) == 0 and not off.any() and g.sizes()[:2] == (65, 0)
    st = g.solve_batch([[0.5, 0.5], [9.0, 9.0]], [[9.5, 9.5], [5.0, 3.9]], [0.5, 1.0])
    assert list(st) == [capi.ERR_NO_SOLUTION_FOUND] * 2
    assert list(g.solve_batch_shortest([[0.5, 0.5]], [[5.0, 3.9]], [1.0])) == [capi.ERR_NO_SOLUTION_FOUND]
    valid, removed = g.revalidate()                      # again, on a roadmap without entries
    assert not valid.any() and removed == 0


def test_thin_sphere_between_two_valid_neighbours():
    states, lists = _shape("two")
    g = capi.PRMRoadmap(2, R2["bounds"], 1.0, 8, lvs_fraction=R2["fraction"])
    g.setup([0.5, 0.5], [9.5, 9.5], 0.5)
    g.set_roadmap(states, *csr(lists))
    g.set_spheres([[1.25, 1.0]], [0.02])
    valid, removed = g.revalidate()
    _, off, nb = g.roadmap()
    assert valid.all() and removed == 2 and len(nb) == 0 and not off.any()


def test_direction_is_construction_s_from_the_higher_index():
    d = fixture()["direction"]
    assert d["found"]
    a, b = unhex_rows([d["a"], d["b"]])
    c, r = unhex_rows([d["sphere"][0]]), [unhex(d["sphere"][1])]
    rrt = capi.RRTBatch(2, d["bounds"], 1.0, 0.05, 1, max_nodes=64, lvs_fraction=d["fraction"])
    rrt.set_spheres(c, r)
    assert list(rrt.is_valid([a, b])) == [True, True]
    assert list(rrt.check_motion([a, b], [b, a])) == [d["a_to_b"], d["b_to_a"]] == [False, True]
    for states, kept in (([a, b], True), ([b, a], False)):   # from = index 1: b -> a is valid, a -> b is not
        g = capi.PRMRoadmap(2, d["bounds"], 1.0, 8, lvs_fraction=d["fraction"])
        g.set_spheres(c, r)
        g.setup([0.5, 0.5], [9.5, 9.5], 0.5)
        g.set_roadmap(states, *csr([[1], [0]]))
        valid, removed = g.revalidate()
        assert valid.all() and removed == (0 if kept else 2)
        assert edge_lists(*g.roadmap()[1:]) == ([[1], [0]] if kept else [[], []])


# ---------------------------------------------------------------------------------------------------------------- Python surface
def test_python_planner_saves_loads_and_revalidates(tmp_path):
    from oxmpl_amd import base
    from oxmpl_amd.geometric import PRM

    class Goal:
        def __init__(self, dim):
            self.target, self.radius = base.RealVectorState([9.0] * dim), 0.8

    def planner(dim, spheres=()):
        space = base.RealVectorStateSpace(dim, [(0.0, 10.0)] * dim)
        pd = base.ProblemDefinition.from_real_vector(space, base.RealVectorState([1.0] * dim), Goal(dim))
        p = PRM(5.0, 1.0, pd, max_milestones=300, seed=4)
        p.setup(base.SphereBoxValidityChecker(spheres=list(spheres)))
        return p

    p = planner(2)
    p.construct_roadmap()
    rm = p.get_roadmap()
    path = str(tmp_path / "roadmap.npz")
    p.save_roadmap(path)
    p2 = planner(2)
    p2.load_roadmap(path)
    assert_roadmap_equal(p2.get_roadmap(), rm)
    assert p2.num_milestones == 300
    with pytest.raises(ValueError):
        planner(3).load_roadmap(path)
    with pytest.raises(ValueError) as e:
        p2.set_roadmap(rm[0], rm[1], rm[2][::-1].copy())
    assert "row" in str(e.value)
    valid, removed = p2.revalidate(base.SphereBoxValidityChecker(spheres=[([5.0, 5.0], 1.5)]))
    assert valid.dtype == bool and 0 < np.count_nonzero(~valid) < 300 and removed > 0
    assert p2.num_milestones == 300 and len(p2.get_roadmap()[2]) == len(rm[2]) - removed
