"""GPU: PRM roadmap construction (prm_kernels.hip, prm_so3.hip) on the scenes of tests/prm_limits_shapes.py, bit for bit against the C
oracle (R^n) and the SO(3) checker: milestone bit patterns, offsets, neighbour lists, sizes() and one query per scene.  What each
scene holds -- refused motions in every dimension, tie rows and short rows, candidates beyond the first buffer, the sample that fills
the roadmap, cones beyond the LDS table, pairs at the band edges -- is held on the CPU by tests/test_prm_limits_model.py; no
expectation here comes from a device run."""
import numpy as np
import pytest

import prm_limits_shapes as shapes
from helpers import bits
from prm_helpers import assert_same_query, assert_same_roadmap, make_gpu_prm
from prm_limits_shapes import g3, gp

pytestmark = pytest.mark.gpu

from oxmpl_amd import capi  # noqa: E402

SO3_STATUS = {capi.OK: "solved", capi.ERR_NO_SOLUTION_FOUND: "no_solution", capi.ERR_INVALID_START_STATE: "invalid_start",
              capi.ERR_UNSAMPLED_STATE_SPACE: "unsampled"}


# ------------------------------------------------------------------------------------------------------------------- R^n
def _build_rn(P, **kw):
    """the device roadmap of P with the scene's query set, and the oracle's"""
    R = shapes.oracle_roadmap(P)
    query = shapes.query_of(P)
    g = make_gpu_prm(P, knn_k=P["knn_k"], **kw)
    g.setup(*query)
    g.construct_roadmap()
    R["o"].set_problem(*query)
    return g, R


def _assert_rn(P, **kw):
    g, R = _build_rn(P, **kw)
    assert_same_roadmap(g, R["o"])
    assert g.sizes() == (R["n"], len(R["nbrs"]), R["n_samples"])
    assert_same_query(g, R["o"])
    return g, R


@pytest.mark.parametrize("knn_k", [0, shapes.RN_KNN])
@pytest.mark.parametrize("dim", shapes.DIMS)
def test_every_dimension_by_radius_and_by_the_nearest(dim, knn_k):
    P = shapes.rn_scene(dim, knn_k)
    g, _ = _assert_rn(P)
    if knn_k:
        m = shapes.knn_model(P)
        assert g.last_timing()["candidates"] == m["candidates"] and g.knn_exact_rows() == m["short_rows"]
    else:
        assert g.last_timing()["candidates"] == shapes.radius_candidates(P)
    g.close()


@pytest.mark.parametrize("knn_k", shapes.GRID_KS)
@pytest.mark.parametrize("frame", list(shapes.GRID_FRAMES))
def test_knn_ties_and_zero_distances_on_a_grid(frame, knn_k):
    P = shapes.grid_scene(frame, knn_k)
    m = shapes.knn_model(P)
    g, _ = _assert_rn(P)
    assert g.knn_exact_rows() == m["short_rows"]
    assert g.last_timing()["candidates"] == m["candidates"]
    g.close()


def test_k_beyond_the_roadmap_takes_every_earlier_milestone():
    """knn_k = 2,000 at 300 milestones: need = min(k, j) = j in every row; the oracle's roadmap, which is the infinite radius's"""
    g, R = _assert_rn(shapes.beyond_scene("knn"))
    assert g.knn_exact_rows() == 0 and g.last_timing()["candidates"] == shapes.BEYOND_N * (shapes.BEYOND_N - 1) // 2
    g2, R2 = _assert_rn(shapes.beyond_scene("radius"))
    for a, b in zip(g.roadmap(), g2.roadmap()):
        assert np.array_equal(a, b)
    g.close()
    g2.close()


def test_knn_search_overflows_the_first_candidate_buffer():
    """3,000 milestones in R^3, k = 120: the per-row radii bring 1,136,691 candidates (the model's count: pairs with d2 <= the
    restated row threshold over the oracle's milestones; k = 80 brings 803,206), more than the 2^20 pairs of find_pairs' first
    buffer, so the pair search runs a second time with the exact size -- through the per-row thresholds"""
    P = shapes.overflow_scene()
    m = shapes.knn_model(P)
    g, _ = _assert_rn(P)
    t = g.last_timing()
    assert t["candidates"] > 2 ** 20 and t["candidates"] == m["candidates"]
    assert g.knn_exact_rows() == m["short_rows"]
    g.close()


def _assert_rebuilds_alike(g, roadmap_of, query):
    """construct_roadmap again: already constructed, nothing moves; setup() restarts the stream: the same roadmap comes back"""
    before, sizes = roadmap_of(g), g.sizes()
    g.construct_roadmap()
    assert g.sizes() == sizes
    g.setup(*query)
    assert g.sizes()[0] == 0
    g.construct_roadmap()
    assert g.sizes() == sizes
    for a, b in zip(before, roadmap_of(g)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_rn_round_ends_at_the_sample_cap(delta):
    """max_samples one below, at and one above the sample S that fills the roadmap (prm_sample_scan_kernel's cut)"""
    S = shapes.rn_fill_samples()
    P = shapes.rn_cut_scene(S + delta)
    g, R = _assert_rn(P)
    assert g.sizes()[0] == (shapes.CUT_N - 1 if delta < 0 else shapes.CUT_N) and g.sizes()[2] == min(S, S + delta)
    _assert_rebuilds_alike(g, lambda x: tuple(bits(a) if a.dtype == np.float64 else a for a in x.roadmap()), shapes.query_of(P))
    assert_same_roadmap(g, R["o"])
    g.close()


# ------------------------------------------------------------------------------------------------------------------ SO(3)
def _make_so3(sc, radius=None, **kw):
    bounds = [0.0, 0.0, 0.0, 1.0, g3.PI] if sc["bounds"] is None else list(sc["bounds"][0]) + [sc["bounds"][1]]
    args = dict(lvs_fraction=sc["fraction"], max_samples=sc["max_samples"], seed=sc["seed"], stream=sc["stream"], space=capi.SPACE_SO3)
    args.update(kw)
    g = capi.PRMRoadmap(4, bounds, sc["radius"] if radius is None else radius, sc["max_milestones"], **args)
    if sc["cones"]:
        g.set_spheres([c for c, _ in sc["cones"]], [r for _, r in sc["cones"]])
    g.setup(*sc["queries"][0])
    return g


def _so3_edges(g):
    states, off, nbrs = g.roadmap()
    return states, [[int(v) for v in nbrs[int(off[i]):int(off[i + 1])]] for i in range(len(states))]


def _assert_so3(g, sc, want, radius=None, query=True):
    """the device roadmap against the checker's: sizes, milestone bits, every edge list, and the scene's first query"""
    states, edges = _so3_edges(g)
    assert g.sizes() == (len(want["states"]), sum(len(e) for e in want["edges"]), want["n_samples"])
    assert np.array_equal(bits(states), bits(want["states"]))
    assert edges == want["edges"]
    assert g.last_timing()["candidates"] == want["candidates"]
    if query and len(states):
        start, target, goal_r = sc["queries"][0]
        rm = dict(states=[[float(v) for v in row] for row in want["states"]], edges=want["edges"])
        status, s_conn, g_idx, path = gp.prm_solve(sc["radius"] if radius is None else radius, sc["fraction"], g3.Cones(sc["cones"]), rm,
                                                   start, target, goal_r)
        st, got = g.solve()
        assert SO3_STATUS.get(st, st) == status
        if status != "invalid_start":
            sc_, gi_ = g.query_sets()
            assert [int(v) for v in sc_] == s_conn and [int(v) for v in gi_] == g_idx
        assert got.shape == (len(path), 4) and np.array_equal(bits(got), bits(np.array(path).reshape(-1, 4)))


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_so3_round_ends_at_the_sample_cap(delta):
    """max_samples one below, at and one above the sample_uniform call S that fills the roadmap: prm_so3_sample_scan_kernel's
    two cuts fall on neighbouring attempts, on one attempt, and S + 1 must not draw further"""
    sc = shapes.so3_cut_scene()
    S = shapes.so3_fill_samples()
    want = shapes.so3_roadmap(sc, max_samples=S + delta)
    g = _make_so3(sc, max_samples=S + delta)
    g.construct_roadmap()
    assert g.sizes()[0] == (shapes.CUT_N - 1 if delta < 0 else shapes.CUT_N) and g.sizes()[2] == min(S, S + delta)
    _assert_so3(g, sc, want)
    _assert_rebuilds_alike(g, lambda x: (bits(x.roadmap()[0]),) + tuple(x.roadmap()[1:]), sc["queries"][0])
    _assert_so3(g, sc, want, query=False)
    g.close()


@pytest.mark.parametrize("count", shapes.CONE_COUNTS)
def test_so3_cone_table_in_lds_and_beyond_it(count):
    """64 cones: the last table prm_so3_edge_kernel<true> holds in LDS; 65 and 130: prm_so3_edge_kernel<false> reads it from memory"""
    sc = shapes.cones_scene(count)
    g = _make_so3(sc)
    g.construct_roadmap()
    _assert_so3(g, sc, shapes.so3_roadmap(sc))
    g.close()


@pytest.mark.parametrize("target", shapes.BAND_TARGETS, ids=str)
def test_so3_radius_one_ulp_either_side_of_a_pair_distance(target):
    sc = shapes.bands_scene()
    j, i, d = shapes.band_pairs()[target]
    for r in shapes.band_radii(d):
        want = shapes.so3_roadmap(sc, radius=r)
        assert (i in want["edges"][j]) == (d < r)
        g = _make_so3(sc, radius=r)
        g.construct_roadmap()
        _assert_so3(g, sc, want, radius=r, query=r == d)
        g.close()


@pytest.mark.parametrize("radius", shapes.BAND_CUTOFF_RADII)
def test_so3_radius_about_the_zero_distance_cut(radius):
    """radii either side of acos(1 - 1e-9): |dot| above 1 - 1e-9 is distance 0 by definition, whatever the radius band says"""
    sc = shapes.bands_scene()
    g = _make_so3(sc, radius=radius)
    g.construct_roadmap()
    _assert_so3(g, sc, shapes.so3_roadmap(sc, radius=radius), radius=radius)
    g.close()
