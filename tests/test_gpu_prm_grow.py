"""GPU: oxhip_prm_grow_roadmap -- a built, planted or re-checked roadmap gets more milestones in place.
Every comparison is bit for bit on (states, offsets, neighbours) and on get_sizes.  The references are code that is already
tested: construct_roadmap itself (growth equals construction), and -- where milestones are dead -- tests/prm_grow_helpers.py's
restatement of the edge rule fed with the RRT batch's is_valid / check_motion and the golden generators' distance (the filter
test_gpu_prm_revalidate.py uses), whose own behaviour tests/test_prm_grow_abi_cpu.py pins on hand-made inputs."""
import math
import os
import sys

import numpy as np
import pytest

from helpers import bits
from prm_grow_helpers import check_rows, expected_growth, make_near, rrt_motion
from prm_revalidate_helpers import edge_lists
from prm_shortest_helpers import Batch, RoadmapChecker, DISTANCE

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden as mg  # noqa: E402
import make_golden_so3 as g3  # noqa: E402

pytestmark = pytest.mark.gpu

from oxmpl_amd import capi  # noqa: E402

SO3_UNBOUNDED = [0.0, 0.0, 0.0, 1.0, math.pi]
FRACTION = 0.05


def _unit(q):
    q = np.asarray(q, dtype=np.float64)
    return (q / np.linalg.norm(q)).tolist()


# scene A of every space, and what scene B adds: a large obstacle that covers milestones and a thin one that only cuts edges
SCENES = {
    "r2": dict(dim=2, radius=0.9, spheres=([[3.0, 3.0], [7.0, 6.0]], [1.0, 0.8]), boxes=([[4.5, 7.0]], [[6.0, 8.5]]),
               more_spheres=([[5.0, 2.0], [1.5, 7.5]], [1.2, 0.15])),
    "r3": dict(dim=3, radius=1.5, spheres=([[3.0, 3.0, 3.0], [7.0, 6.0, 5.0], [2.0, 8.0, 6.0]], [1.2, 1.0, 0.9]),
               boxes=([[4.5, 7.0, 1.0]], [[6.0, 8.5, 3.0]]),
               more_spheres=([[5.0, 5.0, 5.5], [2.0, 6.0, 2.0], [8.0, 2.0, 7.0], [6.5, 1.5, 4.0], [1.5, 2.0, 8.0], [8.0, 8.5, 8.0]],
                             [2.0, 0.6, 0.6, 0.6, 0.6, 0.6])),
    "r6": dict(dim=6, radius=3.5, spheres=([[3.0] * 6, [7.0, 6.0, 5.0, 4.0, 6.0, 7.0]], [2.0, 1.8]),
               boxes=([[0.5, 6.0, 0.5, 6.0, 0.5, 6.0]], [[3.0, 9.5, 3.0, 9.5, 3.0, 9.5]]),
               more_boxes=([[2.5] * 6, [8.0, 1.0, 8.0, 1.0, 8.0, 1.0]], [[7.5] * 6, [8.3, 9.0, 8.3, 9.0, 8.3, 9.0]])),
    "r3_knn": dict(dim=3, radius=1.5, knn_k=5, spheres=([[3.0, 3.0, 3.0], [7.0, 6.0, 5.0]], [1.2, 1.0]),
                   boxes=([[4.5, 7.0, 1.0]], [[6.0, 8.5, 3.0]]), more_spheres=([[5.0, 5.0, 5.5]], [2.0])),
    "so3": dict(dim=4, so3=True, radius=0.3, spheres=([_unit([1, 0, 0, 1]), _unit([0, 1, 1, 0])], [0.35, 0.3]), boxes=([], []),
                more_spheres=([_unit([0, 0, 1, 1]), _unit([1, 1, 1, 1]), _unit([1, -1, 0, 2]), _unit([0, 2, -1, 1]), _unit([3, 0, 1, -1])],
                              [0.5, 0.15, 0.15, 0.15, 0.15])),
}
SEED, STREAM = 20261020, 3


def obstacles(name, scene_b):
    sc = SCENES[name]
    c, r = (list(v) for v in sc["spheres"])
    lo, hi = (list(v) for v in sc["boxes"])
    if scene_b:
        mc, mr = sc.get("more_spheres", ([], []))
        ml, mh = sc.get("more_boxes", ([], []))
        c, r, lo, hi = c + list(mc), r + list(mr), lo + list(ml), hi + list(mh)
    return c, r, lo, hi


def set_obstacles(h, name, scene_b):
    c, r, lo, hi = obstacles(name, scene_b)
    h.set_spheres(np.array(c).reshape(len(r), SCENES[name]["dim"]), r)
    if not SCENES[name].get("so3"):
        h.set_boxes(np.array(lo).reshape(len(lo), SCENES[name]["dim"]), np.array(hi).reshape(len(hi), SCENES[name]["dim"]))


def setup_any(g):
    if g.space == capi.SPACE_SO3:
        g.setup([0.0, 1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], 0.2)
    else:
        g.setup([0.5] * g.dim, [9.5] * g.dim, 0.5)


def prm(name, max_milestones, scene_b=False, stream=STREAM, max_samples=0):
    sc = SCENES[name]
    if sc.get("so3"):
        g = capi.PRMRoadmap(4, SO3_UNBOUNDED, sc["radius"], max_milestones, lvs_fraction=FRACTION, seed=SEED, stream=stream,
                            max_samples=max_samples, space=capi.SPACE_SO3)
    else:
        g = capi.PRMRoadmap(sc["dim"], [(0.0, 10.0)] * sc["dim"], sc["radius"], max_milestones, lvs_fraction=FRACTION, seed=SEED,
                            stream=stream, max_samples=max_samples, knn_k=sc.get("knn_k", 0))
    set_obstacles(g, name, scene_b)
    setup_any(g)
    return g


def rrt(name, scene_b=True):
    """an RRT batch of the scene's space, bounds, fraction and obstacles: the independent is_valid / check_motion"""
    sc = SCENES[name]
    if sc.get("so3"):
        b = capi.RRTBatch(4, SO3_UNBOUNDED, 0.5, 0.05, 1, max_nodes=64, lvs_fraction=FRACTION, space=capi.SPACE_SO3)
    else:
        b = capi.RRTBatch(sc["dim"], [(0.0, 10.0)] * sc["dim"], 1.0, 0.05, 1, max_nodes=64, lvs_fraction=FRACTION)
    set_obstacles(b, name, scene_b)
    return b


def dist_of(name):
    return g3.distance if SCENES[name].get("so3") else mg.distance


def assert_roadmap_equal(a, b):
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def host_expectation(name, old_rows, states, n_old):
    """(live mask, rows after the grow) by the issue's edge rule, from the RRT batch's functions in scene B"""
    b = rrt(name)
    live = b.is_valid(states[:n_old])
    near = make_near(states, n_old, SCENES[name]["radius"], dist_of(name), so3=bool(SCENES[name].get("so3")))
    return live, expected_growth(old_rows, len(states), list(live), near, rrt_motion(b, states))


# ---------------------------------------------------------------------------------------------------------------- 1. growth = construction
_WHOLE = {}


def whole(name, n):
    """the scene's roadmap constructed to n milestones in one call (once per module): (roadmap, sizes)"""
    if (name, n) not in _WHOLE:
        g = prm(name, n)
        g.construct_roadmap()
        _WHOLE[(name, n)] = (g.roadmap(), g.sizes())
        g.close()
    return _WHOLE[(name, n)]


# (N1, then the grows): the wave (63 / 64 / 65), the workgroup (256) and the capacity (1024: the buffers move, the key shift changes)
STEPS = [(1, (1,)), (2, (63,)), (63, (1,)), (64, (64,)), (65, (191,)), (256, (1,)), (300, (300,)), (500, (100, 1, 599)), (1000, (30,))]


@pytest.mark.parametrize("n1,grows", STEPS, ids=["%d+%s" % (a, "+".join(map(str, b))) for a, b in STEPS])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_growth_equals_construction(name, n1, grows):
    g = prm(name, n1)
    g.construct_roadmap()
    assert g.sizes() == whole(name, n1)[1]
    n = n1
    for more in grows:
        before = g.sizes()
        added, drawn = g.grow(more)
        n += more
        want_rm, want_sizes = whole(name, n)
        assert added == more and g.sizes() == want_sizes and drawn == want_sizes[2] - before[2]   # n, n_edge_entries, n_samples
        assert_roadmap_equal(g.roadmap(), want_rm)
    t = g.grow_timing()["phase_ms"]
    assert len(t) == 6 and all(v >= 0.0 for v in t)
    valid, removed = g.revalidate()              # the rule a re-check keeps edges by: nothing goes
    assert valid.all() and removed == 0
    g.close()


# ---------------------------------------------------------------------------------------------------------------- 2. growth after a re-check
_REGROWN = {}
N_A, N_MORE, GENEROUS = 600, 300, 1200


def regrown(name):
    """built in scene A to 600, moved to scene B, re-checked, grown by 300, re-checked again (once per module)"""
    if name not in _REGROWN:
        g = prm(name, N_A)
        g.construct_roadmap()
        rm_a, sizes_a = g.roadmap(), g.sizes()
        set_obstacles(g, name, True)
        valid, removed = g.revalidate()
        g.set_problem(*((([0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0], 0.3)) if SCENES[name].get("so3") else
                        ([9.0] * g.dim, [1.0] * g.dim, 0.7)))          # neither moves the sampler's position
        rm_re, sizes_re = g.roadmap(), g.sizes()
        added, drawn = g.grow(N_MORE)
        rm_g, sizes_g = g.roadmap(), g.sizes()
        valid2, removed2 = g.revalidate()
        _REGROWN[name] = dict(g=g, rm_a=rm_a, sizes_a=sizes_a, valid=valid, removed=removed, rm_re=rm_re, sizes_re=sizes_re, added=added,
                              drawn=drawn, rm_g=rm_g, sizes_g=sizes_g, valid2=valid2, removed2=removed2, rm_after=g.roadmap())
    return _REGROWN[name]


@pytest.mark.parametrize("name", ["r3", "r6", "so3"])
def test_growth_after_a_recheck(name):
    r = regrown(name)
    states, off, nb = r["rm_g"]
    rows_a, rows_re, rows_g = edge_lists(*r["rm_a"][1:]), edge_lists(*r["rm_re"][1:]), edge_lists(off, nb)
    # the scene change does both: invalid milestones, and edges cut between two valid ends
    n_dead = int(np.count_nonzero(~r["valid"]))
    cut = sum(1 for j, row in enumerate(rows_a) for i in row if i < j and r["valid"][i] and r["valid"][j] and i not in rows_re[j])
    assert n_dead > 0 and cut > 0 and r["removed"] > 0
    assert r["added"] == N_MORE and len(states) == N_A + N_MORE
    assert r["sizes_g"] == (N_A + N_MORE, len(nb), r["sizes_a"][2] + r["drawn"]) and r["sizes_re"][2] == r["sizes_a"][2]
    # states: the old ones in place; the new ones a contiguous run of scene B's valid samples of the same stream, beginning where the
    # samples construction drew end
    assert np.array_equal(bits(states[:N_A]), bits(r["rm_a"][0]))
    fresh = prm(name, GENEROUS, scene_b=True)
    fresh.construct_roadmap()
    fs = fresh.roadmap()[0]
    upto = prm(name, GENEROUS, scene_b=True, max_samples=r["sizes_a"][2])   # scene B's milestones among construction's samples
    upto.construct_roadmap()
    first = upto.sizes()[0]
    assert upto.sizes()[2] == r["sizes_a"][2] and first < N_A
    hits = np.nonzero((bits(fs) == bits(states[N_A])).all(axis=1))[0]
    assert len(hits) == 1 and int(hits[0]) == first
    assert np.array_equal(bits(fs[first:first + N_MORE]), bits(states[N_A:]))
    # edges: the host's restatement over the old and the new states
    live, want = host_expectation(name, rows_re, states, N_A)
    assert np.array_equal(live, r["valid"])
    assert rows_g == want
    check_rows(rows_g)
    assert [[v for v in row if v < N_A] for row in rows_g[:N_A]] == rows_re              # the old part of every old row
    assert all(rows_g[i] == [] for i in np.nonzero(~live)[0])                            # a dead milestone got nothing
    assert sum(len(row) for row in rows_g[N_A:]) > N_MORE                                # and the new rows are not empty
    assert any(i < N_A for row in rows_g[N_A:] for i in row)
    # a re-check right after the grow removes nothing
    assert r["removed2"] == 0 and int(np.count_nonzero(~r["valid2"])) == n_dead and r["valid2"][N_A:].all()
    assert_roadmap_equal(r["rm_after"], r["rm_g"])
    fresh.close(); upto.close()


# ---------------------------------------------------------------------------------------------------------------- 3. planted roadmaps
def test_planted_roadmap_needs_a_stream_and_continues_it():
    name = "r2"
    src = prm(name, 300)
    src.construct_roadmap()
    rm = src.roadmap()

    def planted():
        g = prm(name, 300, scene_b=True)          # scene B: some planted milestones are dead, their rows stale (no re-check here)
        g.set_roadmap(*rm)
        return g
    g = planted()
    with pytest.raises(capi.OxhipError) as e:
        g.grow(100)
    assert e.value.status == capi.ERR_BAD_ARG and "OXHIP_PRM_GROW_NEW_STREAM" in str(e.value)
    assert_roadmap_equal(g.roadmap(), rm)
    assert g.sizes() == (300, len(rm[2]), 0)
    assert g.grow(100, new_stream=7)[0] == 100
    ref = prm(name, 100, scene_b=True, stream=7)
    ref.construct_roadmap()
    states, off, nb = g.roadmap()
    assert np.array_equal(bits(states[:300]), bits(rm[0])) and np.array_equal(bits(states[300:]), bits(ref.roadmap()[0]))
    assert g.sizes() == (400, len(nb), ref.sizes()[2])                                   # n_samples counts from 0 after set_roadmap
    live, want = host_expectation(name, edge_lists(*rm[1:]), states, 300)
    assert 0 < np.count_nonzero(~live) < 300 and edge_lists(off, nb) == want
    assert g.grow(50) == (50, g.sizes()[2] - ref.sizes()[2])                             # flags = 0 now continues stream 7
    one = planted()
    assert one.grow(150, new_stream=7) == (150, g.sizes()[2])
    assert_roadmap_equal(one.roadmap(), g.roadmap())
    assert one.sizes() == g.sizes()
    # planting forgets the position even on the handle that constructed the roadmap
    src.set_roadmap(*rm)
    with pytest.raises(capi.OxhipError) as e:
        src.grow(10)
    assert e.value.status == capi.ERR_BAD_ARG and "OXHIP_PRM_GROW_NEW_STREAM" in str(e.value)
    for h in (src, g, ref, one):
        h.close()


# ---------------------------------------------------------------------------------------------------------------- 4. refusals and limits
def _status(fn):
    with pytest.raises(capi.OxhipError) as e:
        fn()
    return e.value.status, str(e.value)


def test_refusals():
    sc = SCENES["r2"]
    g = capi.PRMRoadmap(2, [(0.0, 10.0)] * 2, sc["radius"], 64, lvs_fraction=FRACTION, seed=SEED, stream=STREAM)
    assert _status(lambda: g.grow(4))[0] == capi.ERR_PLANNER_UNINITIALISED
    g.setup([0.5, 0.5], [9.5, 9.5], 0.5)
    st, text = _status(lambda: g.grow(4))
    assert st == capi.ERR_UNSAMPLED_STATE_SPACE and "construct_roadmap" in text
    g.construct_roadmap()
    before, sizes = g.roadmap(), g.sizes()
    assert _status(lambda: g.grow(0))[0] == capi.ERR_BAD_ARG
    assert _status(lambda: g.grow(2 ** 26))[0] == capi.ERR_CAPACITY
    assert_roadmap_equal(g.roadmap(), before)
    assert g.sizes() == sizes
    g.setup([0.5, 0.5], [9.5, 9.5], 0.5)          # setup clears the roadmap: nothing to grow
    assert _status(lambda: g.grow(4))[0] == capi.ERR_UNSAMPLED_STATE_SPACE
    g.close()


def test_k_nearest_growth_over_dead_milestones_is_refused_and_leaves_the_handle():
    name = "r3_knn"
    g = prm(name, 200)
    g.construct_roadmap()
    before, sizes = g.roadmap(), g.sizes()
    set_obstacles(g, name, True)
    assert not rrt(name).is_valid(before[0]).all()
    st, text = _status(lambda: g.grow(10))
    assert st == capi.ERR_BAD_ARG and "not built" in text
    assert_roadmap_equal(g.roadmap(), before)
    assert g.sizes() == sizes
    set_obstacles(g, name, False)                 # back in scene A the refused call has left the stream where it was
    assert g.grow(10)[0] == 10
    want_rm, want_sizes = whole(name, 210)
    assert_roadmap_equal(g.roadmap(), want_rm)
    assert g.sizes() == want_sizes
    g.close()


def test_max_samples_ends_a_grow_that_finds_nothing_valid():
    name = "r2"
    g = prm(name, 100)
    g.construct_roadmap()
    before, sizes = g.roadmap(), g.sizes()
    g.set_spheres([[5.0, 5.0]], [20.0])           # the whole space is covered: the first continued sample, and every other, is invalid
    assert g.grow(1, max_samples=1) == (0, 1)
    assert_roadmap_equal(g.roadmap(), before)
    assert g.sizes() == (sizes[0], sizes[1], sizes[2] + 1)
    assert g.grow(50, max_samples=500) == (0, 500)
    assert_roadmap_equal(g.roadmap(), before)
    assert g.sizes() == (sizes[0], sizes[1], sizes[2] + 501)
    set_obstacles(g, name, False)                 # the samples drawn are spent: the next milestones are later ones of the stream
    assert g.grow(5)[0] == 5
    states = g.roadmap()[0]
    ws = whole(name, 700)[0][0]                   # (its samples reach past the 501 spent ones and the five after them)
    assert whole(name, 700)[1][2] > g.sizes()[2]
    where = [int(np.nonzero((bits(ws) == bits(s)).all(axis=1))[0][0]) for s in states[100:]]
    assert where[0] > 100 and where == list(range(where[0], where[0] + 5))
    g.close()


# ---------------------------------------------------------------------------------------------------------------- 5. services after growth
class Grown(RoadmapChecker):
    def __init__(self, name):
        self.g, self.dist = regrown(name)["g"], dist_of(name)
        self.load_roadmap()


def test_batches_and_single_solves_on_the_grown_roadmap():
    s = Grown("r3")
    rng = np.random.default_rng(23)
    starts, goals, radii = rng.uniform(0.5, 9.5, size=(16, 3)), rng.uniform(0.5, 9.5, size=(16, 3)), np.full(16, 1.2)
    assert s.n == N_A + N_MORE
    B = Batch(s.g, starts, goals, radii, weights=None)
    assert np.count_nonzero(B.status == capi.OK) >= 4
    for q in range(16):                           # the loop a user writes today
        s.g.set_problem(starts[q], goals[q], radii[q])
        st, path = s.g.solve()
        assert st == B.status[q] and np.array_equal(bits(path), bits(B.path(q)))
    S = Batch(s.g, starts, goals, radii, weights=DISTANCE)
    assert np.array_equal(S.status, B.status)
    assert s.check_against_checker(S, DISTANCE) >= 4 and s.compared >= 8
    S.check_rows_are_milestones(s.states)
    assert any(v >= N_A for q in range(16) for v in S.path_nodes(q)[1:])                  # some path uses a milestone the grow added


def test_python_planner_grows_built_and_loaded_roadmaps(tmp_path):
    from oxmpl_amd import base
    from oxmpl_amd.geometric import PRM

    class Goal:
        def __init__(self, dim):
            self.target, self.radius = base.RealVectorState([9.0] * dim), 0.8

    def planner(n, spheres=(([5.0, 5.0], 1.5),)):
        space = base.RealVectorStateSpace(2, [(0.0, 10.0)] * 2)
        pd = base.ProblemDefinition.from_real_vector(space, base.RealVectorState([1.0] * 2), Goal(2))
        p = PRM(5.0, 1.0, pd, max_milestones=n, seed=4)
        p.setup(base.SphereBoxValidityChecker(spheres=list(spheres)))
        return p

    p, whole_p = planner(300), planner(350)
    p.construct_roadmap()
    whole_p.construct_roadmap()
    added, drawn = p.grow_roadmap(50)
    assert added == 50 and drawn > 0 and p.num_milestones == 350
    assert_roadmap_equal(p.get_roadmap(), whole_p.get_roadmap())
    with pytest.raises(ValueError):
        p.grow_roadmap(0)
    with pytest.raises(ValueError):
        p.grow_roadmap(2 ** 26)
    path = str(tmp_path / "roadmap.npz")
    p.save_roadmap(path)
    p2 = planner(350)
    p2.load_roadmap(path)
    with pytest.raises(ValueError) as e:
        p2.grow_roadmap(20)
    assert "OXHIP_PRM_GROW_NEW_STREAM" in str(e.value)
    assert_roadmap_equal(p2.get_roadmap(), p.get_roadmap())
    assert p2.grow_roadmap(20, new_stream=9)[0] == 20 and p2.num_milestones == 370
    s2, o2, n2 = p2.get_roadmap()
    rows = edge_lists(o2, n2)
    check_rows(rows)
    assert np.array_equal(bits(s2[:350]), bits(p.get_roadmap()[0]))
    assert [[v for v in row if v < 350] for row in rows[:350]] == edge_lists(*p.get_roadmap()[1:])
    assert sum(len(r) for r in rows[350:]) > 0
    unset = PRM(5.0, 1.0, planner(8)._pd)
    with pytest.raises(Exception) as e:
        unset.grow_roadmap(5)
    assert "setup() was not called" in str(e.value)
