"""GPU: oxhip_prm_components -- the connected components of a roadmap, labelled on the device.
Each planted case is one set_roadmap, one call and a compare of labels, sizes and summary with the host union-find of
tests/prm_components_shapes.py (whose own rules tests/test_prm_components_model.py holds).  Then real roadmaps -- built,
re-checked, grown -- against the same model over get_roadmap, and the search that already exists (solve_batch) against the
labels: a query is answered iff a start connection and a goal milestone share a label."""
import math

import numpy as np
import pytest

import prm_components_shapes as S
from prm_shortest_helpers import Batch

pytestmark = pytest.mark.gpu

from oxmpl_amd import capi  # noqa: E402
from test_gpu_prm_grow import prm, set_obstacles  # noqa: E402  (the scenes of the grow tests, and a handle over one)

SO3_UNBOUNDED = [0.0, 0.0, 0.0, 1.0, math.pi]
_EXPECTED = {}


def expected(name):
    """the host model's answer for a planted shape, computed once"""
    if name not in _EXPECTED:
        _EXPECTED[name] = S.components(*S.shape(name))
    return _EXPECTED[name]


def handle(n, kind="r2"):
    if kind == "so3":
        g = capi.PRMRoadmap(4, SO3_UNBOUNDED, 0.3, n, space=capi.SPACE_SO3)
        g.setup([0.0, 1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], 0.2)
    elif kind == "knn":
        g = capi.PRMRoadmap(3, [(0.0, 10.0)] * 3, 1.5, n, knn_k=5)
        g.setup([0.5] * 3, [9.5] * 3, 0.5)
    else:
        g = capi.PRMRoadmap(2, [(0.0, 10.0)] * 2, 1.0, n)
        g.setup([0.5] * 2, [9.5] * 2, 0.5)
    return g


def plant(graph, kind="r2"):
    n, off, nb = graph
    g = handle(n, kind)
    g.set_roadmap(S.states_for(n, g.dim, unit=kind == "so3"), off, nb)
    return g


def assert_components(got, want):
    label, size, n_comp, largest_label, largest_size = got
    assert label.dtype == np.uint32 and size.dtype == np.uint32
    assert np.array_equal(label, want[0]) and np.array_equal(size, want[1])
    assert (n_comp, largest_label, largest_size) == tuple(want[2:])


@pytest.mark.parametrize("name", sorted(S.SHAPES))
def test_planted_shape(name):
    g = plant(S.shape(name))
    assert_components(g.components(), expected(name))
    t = g.components_timing()
    assert len(t["phase_ms"]) == 4 and all(v >= 0.0 for v in t["phase_ms"]) and t["launches"] > 0
    g.close()


@pytest.mark.parametrize("kind,name", [("so3", "grid_64x64"), ("knn", "ring_1025"), ("so3", "tie_interleaved"), ("knn", "random_1")])
def test_planted_shape_on_other_handles(kind, name):
    g = plant(S.shape(name), kind)
    assert_components(g.components(), expected(name))
    g.close()


def test_launches_do_not_depend_on_the_graph():
    launches = []
    for graph in (S.shape("chain_65537"), S.shape("star_hub_last"), S.isolated(65537), S.shape("bitrev_chain_65537")):
        g = plant(graph)
        g.components()
        launches.append(g.components_timing()["launches"])
        g.close()
    small = plant(S.shape("one"))
    small.components()
    launches.append(small.components_timing()["launches"])
    small.close()
    assert len(set(launches)) == 1 and launches[0] > 0, launches


def test_null_outputs_capacity_and_refusals():
    import ctypes as C
    L = capi.lib()
    n, off, nb = S.shape("two_cliques")
    g = capi.PRMRoadmap(2, [(0.0, 10.0)] * 2, 1.0, n)
    with pytest.raises(capi.OxhipError) as e:
        g.components()
    assert e.value.status == capi.ERR_PLANNER_UNINITIALISED
    g.setup([0.5] * 2, [9.5] * 2, 0.5)
    with pytest.raises(capi.OxhipError) as e:
        g.components()
    assert e.value.status == capi.ERR_UNSAMPLED_STATE_SPACE
    g.set_roadmap(S.states_for(n, 2), off, nb)
    label = np.full(n, 77, dtype=np.uint32)
    p = label.ctypes.data_as(C.POINTER(C.c_uint32))
    assert L.oxhip_prm_components(g._h, p, None, n - 1, None, None, None) == capi.ERR_CAPACITY
    assert (label == 77).all()
    assert L.oxhip_prm_components(g._h, None, None, 0, None, None, None) == capi.OK            # every out pointer may be NULL
    nc = C.c_uint32()
    assert L.oxhip_prm_components(g._h, None, None, 0, C.byref(nc), None, None) == capi.OK and nc.value == 1
    assert L.oxhip_prm_components(g._h, p, None, n, None, None, None) == capi.OK and np.array_equal(label, expected("two_cliques")[0])
    g.close()


# ---------------------------------------------------------------------------------------------------------------- real roadmaps
def host_components(g):
    states, off, nb = g.roadmap()
    return S.components(len(states), off, nb)


def test_built_rechecked_and_grown_roadmap_and_the_cache():
    g = prm("r2", 600)
    g.construct_roadmap()
    built = host_components(g)
    assert_components(g.components(), built)
    first = g.components_timing()["phase_ms"]
    assert_components(g.components(), built)                       # answered from the labels kept on the device
    again = g.components_timing()["phase_ms"]
    assert again[:3] == [0.0, 0.0, 0.0] and sum(first[:3]) > 0.0
    set_obstacles(g, "r2", True)
    assert_components(g.components(), built)                       # obstacles alone change nothing: only the CSR is read
    valid, removed = g.revalidate()
    assert removed > 0 and not valid.all()
    cut = host_components(g)
    assert cut[2] > built[2]                                       # the re-check cut the roadmap into more pieces ...
    assert_components(g.components(), cut)                         # ... and the kept labels went with the old roadmap
    assert all(cut[1][i] == 1 and cut[0][i] == i for i in np.nonzero(~valid)[0])   # a dead row is a component of its own
    added, _ = g.grow(300)
    assert added == 300
    grown = host_components(g)
    assert_components(g.components(), grown)
    assert grown[2] != cut[2] or not np.array_equal(grown[1][:600], cut[1])
    g.setup([0.5] * 2, [9.5] * 2, 0.5)                             # setup clears the roadmap and everything kept about it
    with pytest.raises(capi.OxhipError) as e:
        g.components()
    assert e.value.status == capi.ERR_UNSAMPLED_STATE_SPACE
    g.close()


def test_planting_drops_the_kept_labels():
    g = plant(S.shape("ring_257"))
    assert_components(g.components(), expected("ring_257"))
    n, off, nb = S.shape("tie_low_first")
    g.set_roadmap(S.states_for(n, 2), off, nb)
    assert_components(g.components(), expected("tie_low_first"))
    g.close()


def test_labels_agree_with_the_batch_search():
    """64 queries on a fragmented roadmap: OXHIP_OK iff a start connection and a goal milestone share a label, and the goal
    milestone reached carries the label of a start connection.  Starts and goal centres are live milestones' own states, so
    no query is refused for its start and both sets are never empty: the outcome is the roadmap's connectivity alone."""
    g = prm("r2", 200)
    g.construct_roadmap()
    set_obstacles(g, "r2", True)
    valid, _ = g.revalidate()
    states = g.roadmap()[0]
    label, size, n_comp, _, largest = g.components()
    live = np.nonzero(valid)[0]
    rng = np.random.default_rng(5)
    a, b = rng.choice(live, 64), rng.choice(live, 64)
    B = Batch(g, states[a], states[b], np.full(64, 0.3), weights=None)
    outcomes = set()
    for q in range(64):
        sc, gi = g.batch_query_sets(q)
        assert a[q] in sc and b[q] in gi
        shared = bool(set(label[sc].tolist()) & set(label[gi].tolist()))
        assert (B.status[q] == capi.OK) == shared, q
        assert B.status[q] in (capi.OK, capi.ERR_NO_SOLUTION_FOUND)
        if shared:
            assert label[B.goal[q]] in set(label[sc].tolist())
        outcomes.add(int(B.status[q]))
    print("components %d, largest %d of %d; answered %d of 64" % (n_comp, largest, len(states), int(np.count_nonzero(B.status == capi.OK))))
    assert outcomes == {capi.OK, capi.ERR_NO_SOLUTION_FOUND}
    assert_components((label, size, n_comp, g.components()[3], largest), host_components(g))
    g.close()


def test_python_planner_has_components():
    from oxmpl_amd import base
    from oxmpl_amd.geometric import PRM

    class Goal:
        def __init__(self):
            self.target, self.radius = base.RealVectorState([9.0, 9.0]), 0.8

    space = base.RealVectorStateSpace(2, [(0.0, 10.0)] * 2)
    pd = base.ProblemDefinition.from_real_vector(space, base.RealVectorState([1.0, 1.0]), Goal())
    p = PRM(5.0, 0.8, pd, max_milestones=300, seed=4)
    p.setup(base.SphereBoxValidityChecker(spheres=[([5.0, 5.0], 1.5)]))
    p.construct_roadmap()
    states, off, nb = p.get_roadmap()
    assert_components(p.components(), S.components(len(states), off, nb))
