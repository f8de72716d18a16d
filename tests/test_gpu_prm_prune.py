"""GPU: oxhip_prm_prune -- milestones removed, the rest renumbered in their old order.
After every call get_roadmap is compared bit for bit with host_prune (tests/prm_components_shapes.py, held to its rules by
tests/test_prm_components_model.py) of the roadmap before: states as bit patterns, offsets, neighbours, new_index, n_kept and
n_removed_entries.  The stage-1 mask of an INVALID prune comes from an RRT batch's is_valid over the same space and obstacles."""
import ctypes as C
import math

import numpy as np
import pytest

import prm_components_shapes as S
from helpers import bits
from prm_grow_helpers import check_rows, expected_growth, rrt_motion
from prm_revalidate_helpers import edge_lists
from prm_shortest_helpers import Batch, DISTANCE

pytestmark = pytest.mark.gpu

from oxmpl_amd import capi  # noqa: E402
from test_gpu_prm_grow import SCENES, prm, rrt, set_obstacles, whole  # noqa: E402  (the scenes of the grow tests)

SO3_UNBOUNDED = [0.0, 0.0, 0.0, 1.0, math.pi]


def handle(n, kind):
    """an empty handle after setup(): kind = "so3", "knn" or the dimension of an R^n radius handle"""
    if kind == "so3":
        g = capi.PRMRoadmap(4, SO3_UNBOUNDED, 0.3, n, space=capi.SPACE_SO3)
        g.setup([0.0, 1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], 0.2)
    elif kind == "knn":
        g = capi.PRMRoadmap(3, [(0.0, 10.0)] * 3, 1.5, n, knn_k=5)
        g.setup([0.5] * 3, [9.5] * 3, 0.5)
    else:
        g = capi.PRMRoadmap(kind, [(0.0, 10.0)] * kind, 1.0, n)
        g.setup([0.5] * kind, [9.5] * kind, 0.5)
    return g


def plant(graph, kind=2, states=None):
    n, off, nb = graph
    g = handle(n, kind)
    g.set_roadmap(S.states_for(n, g.dim, unit=kind == "so3") if states is None else states, off, nb)
    return g


def check_prune(g, stage1_keep, invalid=False, keep=None, min_size=0, largest=False):
    """one prune against host_prune of the roadmap before it; returns host_prune's result"""
    before, sizes = g.roadmap(), g.sizes()
    want = S.host_prune(before[0], before[1], before[2], stage1_keep, min_size=min_size, largest=largest)
    new_index, n_kept, removed = g.prune(invalid=invalid, keep=keep, min_size=min_size, largest=largest)
    states, off, nb = g.roadmap()
    assert new_index.dtype == np.int32 and np.array_equal(new_index, want["new_index"])
    assert (n_kept, removed) == (want["n_kept"], want["n_removed_entries"])
    assert states.shape == want["states"].shape and np.array_equal(bits(states), bits(want["states"]))
    assert np.array_equal(off, want["offsets"]) and np.array_equal(nb, want["nbrs"])
    assert g.sizes() == (n_kept, len(want["nbrs"]), sizes[2])               # n_samples stays
    kept = new_index[new_index >= 0]
    assert np.array_equal(kept, np.arange(n_kept))                          # monotone: survivors keep their order
    t = g.prune_timing()["phase_ms"]
    assert len(t) == 5 and all(v >= 0.0 for v in t)
    return want


def built(name, n, scene_b=True):
    """the scene's roadmap built under scene A; the handle then holds scene B's obstacles (the rows are stale: no re-check)"""
    g = prm(name, n)
    g.construct_roadmap()
    if scene_b:
        set_obstacles(g, name, True)
    return g


def valid_now(name, g):
    return np.asarray(rrt(name).is_valid(g.roadmap()[0]), dtype=bool)


# ---------------------------------------------------------------------------------------------------------------- each flag alone
@pytest.mark.parametrize("name", ["r2", "r3", "r6", "so3", "r3_knn"])
def test_invalid_alone(name):
    g = built(name, 600)
    valid = valid_now(name, g)
    assert 0 < np.count_nonzero(~valid) < 600
    want = check_prune(g, valid, invalid=True)
    assert want["n_removed_entries"] > 0
    valid2, removed2 = g.revalidate()                                       # every survivor is valid; revalidate may still cut edges
    assert valid2.all() and len(valid2) == want["n_kept"]
    g.close()


MASKS = {
    "first": lambda n: np.arange(n) != 0,
    "last": lambda n: np.arange(n) != n - 1,
    "every_second": lambda n: np.arange(n) % 2 == 0,
    "all_but_one": lambda n: np.arange(n) == n // 3,
    "none_dropped": lambda n: np.ones(n, dtype=bool),
    "random": lambda n: np.random.default_rng(n).random(n) < 0.7,
}


@pytest.mark.parametrize("mask", sorted(MASKS))
@pytest.mark.parametrize("name", ["ring_257", "grid_64x64", "two_cliques"])
def test_mask_alone(name, mask):
    g = plant(S.shape(name))
    keep = MASKS[mask](S.shape(name)[0])
    check_prune(g, keep, keep=keep)
    g.close()


@pytest.mark.parametrize("kind", [1, 3, 8, "so3", "knn"])
def test_mask_on_every_kind_of_handle(kind):
    name = "random_2"
    g = plant(S.shape(name), kind)
    keep = np.random.default_rng(3).random(S.shape(name)[0]) < 0.6
    want = check_prune(g, keep, keep=keep)
    label = g.components()[0]                                               # the pruned roadmap is a roadmap: its components are the model's
    assert np.array_equal(label, S.components(want["n_kept"], want["offsets"], want["nbrs"])[0])
    g.close()


@pytest.mark.parametrize("k", [255, 256, 257])
def test_n_kept_around_a_workgroup(k):
    n = S.shape("ring_1025")[0]
    keep = np.zeros(n, dtype=bool)
    keep[np.random.default_rng(k).choice(n, k, replace=False)] = True
    g = plant(S.shape("ring_1025"))
    assert check_prune(g, keep, keep=keep)["n_kept"] == k
    g.close()


@pytest.mark.parametrize("k", [128, 129, 130])
def test_kept_entries_around_a_workgroup(k):
    """a chain's first k milestones keep 2 (k - 1) entries: 254, 256, 258 (entries come in mirrored pairs, so these are the
    counts next to 256)"""
    n = 1025
    keep = np.arange(n) < k
    g = plant(S.chain(n))
    want = check_prune(g, keep, keep=keep)
    assert len(want["nbrs"]) == 2 * (k - 1)
    g.close()


def test_min_size_alone():
    name = "random_1"
    n, off, nb = S.shape(name)
    g = plant(S.shape(name))
    everyone = np.ones(n, dtype=bool)
    same = check_prune(g, everyone, min_size=1)                             # a no-op that still returns the identity map
    assert np.array_equal(same["new_index"], np.arange(n)) and same["n_removed_entries"] == 0
    two = check_prune(g, everyone, min_size=2)                              # exactly the rows without entries go
    assert np.array_equal(two["new_index"] < 0, np.diff(off.astype(np.int64)) == 0) and two["n_removed_entries"] == 0
    big = check_prune(g, np.ones(two["n_kept"], dtype=bool), min_size=20)
    assert 0 < big["n_kept"] < two["n_kept"]
    g.close()


@pytest.mark.parametrize("name", ["tie_low_first", "tie_interleaved", "random_1", "random_0.5", "star_hub_last"])
def test_largest_alone_and_its_ties(name):
    n = S.shape(name)[0]
    g = plant(S.shape(name))
    want = check_prune(g, np.ones(n, dtype=bool), largest=True)
    _, _, _, largest_label, largest_size = S.components(*S.shape(name))
    assert want["n_kept"] == largest_size and want["new_index"][largest_label] == 0   # ties: the lowest label's component stays
    assert g.components()[2:] == (1, 0, largest_size)
    g.close()


# ---------------------------------------------------------------------------------------------------------------- combinations
def test_invalid_and_mask():
    g = built("r2", 600)
    valid = valid_now("r2", g)
    mask = np.random.default_rng(8).random(600) < 0.8
    assert np.count_nonzero(valid & ~mask) and np.count_nonzero(~valid & mask) and np.count_nonzero(~valid & ~mask)
    check_prune(g, valid & mask, invalid=True, keep=mask)
    g.close()


def test_mask_and_min_size():
    name = "random_2"
    n = S.shape(name)[0]
    mask = np.random.default_rng(9).random(n) < 0.5
    g = plant(S.shape(name))
    want = check_prune(g, mask, keep=mask, min_size=3)                      # sizes are those of the masked graph, not of the planted one
    whole_graph = S.host_prune(S.states_for(n, 2), *S.shape(name)[1:], np.ones(n, dtype=bool), min_size=3)
    assert want["n_kept"] < np.count_nonzero(mask & (whole_graph["new_index"] >= 0))
    g.close()


def test_invalid_and_largest_on_the_cut_vertex():
    """the cut milestone lies in a sphere: INVALID drops it and LARGEST, evaluated on what is left, drops the path behind it"""
    n, off, nb = S.shape("cut_vertex")
    states = np.array([[1.0 + 0.2 * i, 1.0 + 0.1 * (i % 2)] for i in range(6)] + [[5.0, 5.0], [8.0, 8.0], [8.5, 8.0], [9.0, 8.0]])
    g = plant(S.shape("cut_vertex"), 2, states)
    g.set_spheres([[5.0, 5.0]], [0.5])
    alive = np.ones(n, dtype=bool)
    alive[S.CUT] = False
    want = check_prune(g, alive, invalid=True, largest=True)
    assert want["new_index"].tolist() == [0, 1, 2, 3, 4, 5, -1, -1, -1, -1]
    g.close()
    g = plant(S.shape("cut_vertex"), 2, states)                             # without the sphere nothing is invalid: all ten stay
    assert check_prune(g, np.ones(n, dtype=bool), invalid=True, largest=True)["n_kept"] == 10
    g.close()


def test_all_four_flags():
    g = built("r2", 150)                                                    # sparse enough to lie in several pieces
    valid = valid_now("r2", g)
    mask = np.random.default_rng(10).random(150) < 0.85
    want = check_prune(g, valid & mask, invalid=True, keep=mask, min_size=2, largest=True)
    assert 2 <= want["n_kept"] < np.count_nonzero(valid & mask)
    assert g.components()[2] == 1
    g.close()


# ---------------------------------------------------------------------------------------------------------------- refusals
def _queries(dim, q=64, seed=21):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 9.5, size=(q, dim)), rng.uniform(0.5, 9.5, size=(q, dim)), np.full(q, 1.0)


def test_every_refusal_leaves_the_handle_as_it_was():
    L = capi.lib()
    g = built("r2", 300)
    before, sizes = g.roadmap(), g.sizes()
    queries = _queries(2)
    B0 = Batch(g, *queries, weights=None)
    n = sizes[0]
    ones = np.ones(n, dtype=np.uint8)
    p_ones = ones.ctypes.data_as(C.POINTER(C.c_uint8))

    def raw(flags, min_size=0, pad=0, struct_size=16, keep=None):
        c = capi.PrmPruneConfig()
        c.struct_size, c.flags, c.min_size, c.pad = struct_size, flags, min_size, pad
        return L.oxhip_prm_prune(g._h, C.byref(c), keep, None, None, None), L.oxhip_last_error_string()
    for args in (dict(flags=0), dict(flags=16), dict(flags=1, pad=3), dict(flags=1, struct_size=12), dict(flags=capi.PRM_PRUNE_MASK),
                 dict(flags=capi.PRM_PRUNE_INVALID, keep=p_ones), dict(flags=capi.PRM_PRUNE_MIN_SIZE)):
        assert raw(**args)[0] == capi.ERR_BAD_ARG, args
    assert L.oxhip_prm_prune(g._h, None, None, None, None, None) == capi.ERR_BAD_ARG
    zeros = np.zeros(n, dtype=np.uint8)
    for args in (dict(flags=capi.PRM_PRUNE_MASK, keep=zeros.ctypes.data_as(C.POINTER(C.c_uint8))),
                 dict(flags=capi.PRM_PRUNE_MIN_SIZE, min_size=n + 1),
                 dict(flags=capi.PRM_PRUNE_MASK | capi.PRM_PRUNE_LARGEST, keep=zeros.ctypes.data_as(C.POINTER(C.c_uint8)))):
        st, text = raw(**args)
        assert st == capi.ERR_BAD_ARG and b"would keep no milestone" in text, args
    with pytest.raises(capi.OxhipError):
        g.prune(keep=np.ones(n - 1, dtype=bool))
    after = g.roadmap()
    assert np.array_equal(bits(after[0]), bits(before[0])) and np.array_equal(after[1], before[1]) and np.array_equal(after[2], before[2])
    assert g.sizes() == sizes
    Batch(g, *queries, weights=None).same_as(B0)
    assert raw(capi.PRM_PRUNE_MIN_SIZE, min_size=1)[0] == capi.OK           # NULL outputs are fine on a call that runs
    assert g.sizes() == sizes
    g.close()
    h = capi.PRMRoadmap(2, [(0.0, 10.0)] * 2, 1.0, 64)
    with pytest.raises(capi.OxhipError) as e:
        h.prune(largest=True)
    assert e.value.status == capi.ERR_PLANNER_UNINITIALISED
    h.setup([0.5] * 2, [9.5] * 2, 0.5)
    with pytest.raises(capi.OxhipError) as e:
        h.prune(largest=True)
    assert e.value.status == capi.ERR_UNSAMPLED_STATE_SPACE
    h.close()


# ---------------------------------------------------------------------------------------------------------------- what follows a prune
def _knn_near(states, n_old, k):
    """near(j, i) of a k-nearest handle: i is one of the k nearest earlier milestones of the new milestone j"""
    s = np.asarray(states, dtype=np.float64)
    chosen = {}
    for j in range(n_old, len(s)):
        d2 = ((s[:j] - s[j]) ** 2).sum(axis=1)
        chosen[j] = set(np.argsort(d2, kind="stable")[:k].tolist())
    return lambda j, i: i in chosen[j]


def test_k_nearest_roadmap_grows_again_after_a_prune():
    name = "r3_knn"
    g = built(name, 200)
    g.revalidate()
    with pytest.raises(capi.OxhipError) as e:
        g.grow(40)
    assert e.value.status == capi.ERR_BAD_ARG and "not built" in str(e.value)
    valid = valid_now(name, g)
    want = check_prune(g, valid, invalid=True)
    n_old = want["n_kept"]
    assert n_old < 200
    old_rows = edge_lists(want["offsets"], want["nbrs"])
    added, _ = g.grow(40)
    assert added == 40
    states, off, nb = g.roadmap()
    assert np.array_equal(bits(states[:n_old]), bits(want["states"]))
    rows = edge_lists(off, nb)
    expect = expected_growth(old_rows, len(states), [True] * n_old, _knn_near(states, n_old, SCENES[name]["knn_k"]), rrt_motion(rrt(name), states))
    assert rows == expect
    check_rows(rows)
    assert g.revalidate()[0].all()
    g.close()


def test_prune_then_revalidate_finds_no_invalid_milestone():
    for name in ("r3", "so3"):
        g = built(name, 400)
        g.prune(invalid=True)
        valid, _ = g.revalidate()
        assert valid.all()
        g.close()


def test_the_sampler_continues_where_it_stood():
    name, n1, n2 = "r2", 300, 100
    g = prm(name, n1)
    g.construct_roadmap()
    mask = np.random.default_rng(12).random(n1) < 0.6
    want = check_prune(g, mask, keep=mask)
    assert g.grow(n2) == (n2, whole(name, n1 + n2)[1][2] - whole(name, n1)[1][2])
    states = g.roadmap()[0]
    assert len(states) == want["n_kept"] + n2
    assert np.array_equal(bits(states[want["n_kept"]:]), bits(whole(name, n1 + n2)[0][0][n1:]))
    assert g.sizes()[2] == whole(name, n1 + n2)[1][2]
    g.close()


@pytest.mark.parametrize("name", ["r3", "so3"])
def test_pruned_handle_and_planted_twin_answer_alike(name):
    g = built(name, 500)
    valid = valid_now(name, g)
    mask = np.random.default_rng(13).random(500) < 0.9
    want = check_prune(g, valid & mask, invalid=True, keep=mask, min_size=2)
    twin = prm(name, 500, scene_b=True)
    twin.set_roadmap(want["states"], want["offsets"], want["nbrs"])
    live = want["states"]
    rng = np.random.default_rng(14)
    a, b = rng.choice(len(live), 64), rng.choice(len(live), 64)
    jitter = 0.0 if SCENES[name].get("so3") else rng.uniform(-0.05, 0.05, size=(64, g.dim))
    starts, goals, radii = live[a] + jitter, live[b], np.full(64, 0.25 if SCENES[name].get("so3") else 1.0)
    B, T = Batch(g, starts, goals, radii, weights=None), Batch(twin, starts, goals, radii, weights=None)
    B.same_as(T)
    assert np.count_nonzero(B.status == capi.OK) >= 4
    Bs, Ts = Batch(g, starts, goals, radii, weights=DISTANCE), Batch(twin, starts, goals, radii, weights=DISTANCE)
    Bs.same_as(Ts)
    assert np.array_equal(Bs.status, B.status)
    g.close(); twin.close()


def test_python_planner_prunes():
    from oxmpl_amd import base
    from oxmpl_amd.geometric import PRM

    class Goal:
        def __init__(self):
            self.target, self.radius = base.RealVectorState([9.0, 9.0]), 0.8

    space = base.RealVectorStateSpace(2, [(0.0, 10.0)] * 2)
    pd = base.ProblemDefinition.from_real_vector(space, base.RealVectorState([1.0, 1.0]), Goal())
    p = PRM(5.0, 0.6, pd, max_milestones=300, seed=4)
    p.setup(base.SphereBoxValidityChecker(spheres=[([5.0, 5.0], 1.5)]))
    p.construct_roadmap()
    states, off, nb = p.get_roadmap()
    want = S.host_prune(states, off, nb, np.ones(len(states), dtype=bool), largest=True)
    new_index, n_kept, removed = p.prune_roadmap(largest=True)
    assert np.array_equal(new_index, want["new_index"]) and (n_kept, removed) == (want["n_kept"], want["n_removed_entries"])
    assert p.num_milestones == n_kept and p.components()[2] == 1
    with pytest.raises(ValueError) as e:
        p.prune_roadmap(min_size=10 ** 6)
    assert "would keep no milestone" in str(e.value)
    with pytest.raises(ValueError):
        p.prune_roadmap(keep=np.zeros(n_kept, dtype=bool))
    assert p.num_milestones == n_kept
