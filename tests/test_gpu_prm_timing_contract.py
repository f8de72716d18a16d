"""GPU: what the PRM handle's phase times and counters mean (oxhip_prm_api.hip), pinned so that a change to how they are kept cannot
move them unseen.  One handle per space goes through every service in order -- construct, solve, solve_batch, three shortest-path
batches, revalidate, grow, components twice, two prunes -- and after every call each service's array is compared bit for bit with
what it was before: a call writes its own array and no other.  The exceptions are stated where they are asserted.  No phase time is
compared with a duration; only lengths, finiteness, sign, exact zeros and bitwise (in)equality between getters are.

Counters: with no dead milestone, last_timing()["candidates"] after a grow is construction's in-radius pairs plus growth's, so it
equals the in-radius pairs among all states; knn_exact_rows() after a grow is likewise construction's rows plus growth's.  Both are
counted here on the CPU from the states the handle returns, after a check that no distance lies within 1e-9 relative of a threshold."""
import math

import numpy as np
import pytest

from prm_limits_shapes import earlier, pair_d2

pytestmark = pytest.mark.gpu

from oxmpl_amd import capi, scenarios  # noqa: E402

N0, MORE, Q, CHUNK = 200, 56, 5, 2     # 256 milestones at the most; 5 queries in rounds of 2: 3 rounds
MARGIN = 1e-9
SO3_UNBOUNDED = [0.0, 0.0, 0.0, 1.0, math.pi]
# mean degree about 8: R^3, 200 milestones in 10^3: 200 * (4/3) PI r^3 / 1000 = 8 at r = 2.1 (less near the faces);
# SO(3), volume PI^2 under acos|dot|: 200 * (4/3) PI r^3 / PI^2 = 8 at r = 0.455
R3 = dict(dim=3, bounds=[(0.0, 10.0)] * 3, connection_radius=2.0, lvs_fraction=0.05, max_milestones=N0, start=[1.0, 1.0, 1.0],
          goal_centre=[9.0, 9.0, 9.0], goal_radius=1.5, boxes=None,
          spheres=([[5.0, 5.0, 5.0], [2.5, 7.0, 3.0], [7.5, 3.0, 6.5]], [1.5, 1.0, 1.2]))
SO3_RADIUS = 0.45
SO3_CONES = ([[1.0, 0.0, 0.0, 0.0], [0.0, 0.6, 0.0, 0.8], [0.5, 0.5, 0.5, -0.5]], [0.3, 0.25, 0.3])

SERVICES = ("construct", "batch", "stats", "revalidate", "grow", "components", "prune")
LENGTHS = dict(construct=6, batch=4, stats=6, revalidate=4, grow=6, components=4, prune=5)


SO3_QUERY = ([0.0, 0.0, 0.0, 1.0], [0.0, 1.0, 0.0, 0.0], 0.4)


def make(kind):
    if kind == "so3":
        g = capi.PRMRoadmap(4, SO3_UNBOUNDED, SO3_RADIUS, N0, space=capi.SPACE_SO3)
        g.set_spheres(*SO3_CONES)
        g.setup(*SO3_QUERY)
        return g
    return scenarios.make_prm(R3)


def phases(g):
    """every service's phase array as the getters return it (the search stats: their refusal's status where they refuse)"""
    out = dict(construct=g.last_timing()["phase_ms"], batch=g.batch_last_timing()["phase_ms"],
               revalidate=g.revalidate_last_timing()["phase_ms"], grow=g.grow_timing()["phase_ms"],
               components=g.components_timing()["phase_ms"], prune=g.prune_timing()["phase_ms"])
    try:
        out["stats"] = g.batch_search_stats()["phase_ms"]
    except capi.OxhipError as e:
        out["stats"] = e.status
    for name, ms in out.items():
        if isinstance(ms, list):
            assert len(ms) == LENGTHS[name] and all(math.isfinite(v) and v >= 0.0 for v in ms), (name, ms)
    return out


def bits(ms):
    return ms if isinstance(ms, int) else np.array(ms, dtype=np.float64).tobytes()


def step(g, name, call, own):
    """runs `call`; every service's array outside `own` is bitwise what it was.  -> (the call's result, phases before, after)"""
    before = phases(g)
    result = call()
    after = phases(g)
    print(name, {k: after[k] for k in own})
    for s in SERVICES:
        if s not in own:
            assert bits(after[s]) == bits(before[s]), (name, s, before[s], after[s])
    return result, before, after


def in_radius_pairs(states, radius, so3):
    """pairs (j, i < j) with distance < radius, and the proof that rounding cannot move one across the threshold"""
    low = earlier(len(states))
    if so3:
        dot = np.abs(states @ states.T)
        d = np.where(dot > 1.0 - 1e-9, 0.0, np.arccos(np.minimum(dot, 1.0)))
        assert (np.abs(d[low] - radius) > MARGIN * radius).all()
    else:
        d2 = pair_d2(states)
        assert (np.abs(d2[low] - radius * radius) > MARGIN * radius * radius).all()
        d = np.sqrt(d2)
    return int(((d < radius) & low).sum())


def queries(g):
    """Q queries from milestones to balls about other milestones: every start is valid"""
    states = g.roadmap()[0]
    idx = np.arange(Q)
    return states[idx * 7 % len(states)], states[(idx * 31 + 100) % len(states)], np.full(Q, 0.5 * (SO3_RADIUS if g.space else 1.0))


@pytest.mark.parametrize("kind", ["r3", "so3"])
def test_each_call_writes_its_own_phase_times(kind):
    g = make(kind)
    so3 = kind == "so3"
    radius = SO3_RADIUS if so3 else R3["connection_radius"]
    first = phases(g)
    assert all(bits(first[s]) == bytes(8 * LENGTHS[s]) for s in SERVICES if s != "stats")
    assert first["stats"] == capi.ERR_UNSAMPLED_STATE_SPACE                      # no batch yet

    _, _, t = step(g, "construct", g.construct_roadmap, {"construct"})
    assert t["construct"][4] == 0.0 and t["construct"][5] == 0.0                 # no query yet
    assert g.sizes()[0] == N0
    states0 = g.roadmap()[0]
    assert g.last_timing()["candidates"] == in_radius_pairs(states0, radius, so3)
    n_edges = g.sizes()[1]
    print(kind, "mean degree", n_edges / N0)
    assert 2.0 < n_edges / N0 < 20.0                                             # (the scene, not the library: a degree near 8)

    _, b, t = step(g, "solve", g.solve, {"construct"})
    assert bits(t["construct"][:4]) == bits(b["construct"][:4])                  # a solve writes entries 4 and 5 only

    # the roadmap cleared and built again on the same handle: all six entries start over, the last solve's two included
    step(g, "setup", lambda: g.setup(*(SO3_QUERY if so3 else (R3["start"], R3["goal_centre"], R3["goal_radius"]))), set())
    _, _, t = step(g, "construct again", g.construct_roadmap, {"construct"})
    assert t["construct"][4] == 0.0 and t["construct"][5] == 0.0
    assert np.array_equal(g.roadmap()[0], states0)                               # (the same stream from its start: the same roadmap)
    step(g, "solve again", g.solve, {"construct"})

    starts, goals, radii = queries(g)
    _, _, t = step(g, "solve_batch", lambda: g.solve_batch(starts, goals, radii, chunk_queries=CHUNK), {"batch", "stats"})
    assert g.batch_last_timing()["rounds"] == 3
    assert t["stats"] == capi.ERR_BAD_ARG                                        # the last batch was not a shortest-path batch
    step(g, "batch_query_sets", lambda: g.batch_query_sets(1), set())

    for i, weights in enumerate((0, 0, 1)):
        _, _, t = step(g, "shortest %d" % i, lambda: g.solve_batch_shortest(starts, goals, radii, chunk_queries=CHUNK, weights=weights),
                       {"batch", "stats"})
        assert g.batch_last_timing()["rounds"] == 3
        assert bits([t["stats"][1], t["stats"][4], t["stats"][5]]) == bits([t["batch"][0], t["batch"][2], t["batch"][3]])
        if i:
            assert t["stats"][0] == 0.0       # the weights exist (second batch on this roadmap) or are not needed (unit weights)
        step(g, "batch_labels %d" % i, lambda: g.batch_labels(1), set())
        step(g, "batch_query_sets %d" % i, lambda: g.batch_query_sets(1), set())

    # a batch of either kind resets both arrays before it runs: one without queries leaves them at zero
    none = np.zeros((0, g.dim))
    _, _, t = step(g, "shortest, no queries", lambda: g.solve_batch_shortest(none, none, np.zeros(0), weights=0), {"batch", "stats"})
    assert bits(t["batch"]) == bytes(32) and bits(t["stats"]) == bytes(48) and g.batch_last_timing()["rounds"] == 0
    step(g, "shortest again", lambda: g.solve_batch_shortest(starts, goals, radii, chunk_queries=CHUNK, weights=1), {"batch", "stats"})
    _, _, t = step(g, "breadth-first, no queries", lambda: g.solve_batch(none, none, np.zeros(0)), {"batch", "stats"})
    assert bits(t["batch"]) == bytes(32) and t["stats"] == capi.ERR_BAD_ARG and g.batch_last_timing()["rounds"] == 0
    step(g, "shortest once more", lambda: g.solve_batch_shortest(starts, goals, radii, chunk_queries=CHUNK, weights=1), {"batch", "stats"})

    # a call that changes the roadmap forgets the last batch: its search stats refuse from here on, its batch_ms stays readable
    (valid, removed), _, t = step(g, "revalidate", g.revalidate, {"revalidate", "stats"})
    assert t["stats"] == capi.ERR_UNSAMPLED_STATE_SPACE and valid.all()          # same obstacles: no dead milestone

    c0 = g.last_timing()["candidates"]
    (added, _), b, t = step(g, "grow", lambda: g.grow(MORE), {"grow"})
    assert added == MORE and bits(t["construct"]) == bits(b["construct"])
    states1 = g.roadmap()[0]
    assert np.array_equal(states1[:N0], states0)
    assert c0 == in_radius_pairs(states1[:N0], radius, so3)
    assert g.last_timing()["candidates"] == in_radius_pairs(states1, radius, so3)   # construction's pairs plus growth's

    _, _, t = step(g, "components", g.components, {"components"})
    launches = g.components_timing()["launches"]
    _, _, t = step(g, "components again", g.components, {"components"})
    assert t["components"][:3] == [0.0, 0.0, 0.0] and g.components_timing()["launches"] == launches   # the labels were kept

    (_, kept, _), _, t = step(g, "prune invalid", lambda: g.prune(invalid=True), {"prune"})
    assert kept == N0 + MORE and t["prune"][1] == 0.0                            # no stage 2: no components
    step(g, "prune largest", lambda: g.prune(largest=True), {"prune"})
    g.close()


def knn_rows(states, j0, j1, n_samples, k):
    """(candidate pairs, rows searched exactly) of the rows [j0, j1) in one round that ends with j1 milestones after n_samples
    samples: knn_row_radii's radius per row, the pairs within it, and the rows that hold fewer than min(k, j) of them"""
    dim = states.shape[1]
    vol = 10.0 ** dim
    frac = min(1.0, j1 / n_samples)
    c_d = math.pow(math.pi, 0.5 * dim) / math.gamma(0.5 * dim + 1.0)
    want = 6.0 * k
    d2 = pair_d2(states)
    cand = exact = 0
    for j in range(max(j0, 1), j1):
        if j <= want:
            cand += j
            continue
        r = math.pow(want * vol * frac / (c_d * j), 1.0 / dim)
        assert (np.abs(d2[j, :j] - r * r) > MARGIN * r * r).all()
        hits = int((d2[j, :j] <= r * r).sum())
        cand += hits
        exact += hits < min(k, j)
    return cand, exact


def test_knn_counters_across_a_grow():
    k, n0, more = 4, 64, 192   # (split where both calls have rows that fall short: their radii reach past the box's corners)
    g = scenarios.make_prm(R3, max_milestones=n0, knn_k=k)
    g.construct_roadmap()
    samples0 = g.sizes()[2]
    assert g.sizes()[0] == n0
    c0, e0 = knn_rows(g.roadmap()[0], 0, n0, samples0, k)
    assert (g.last_timing()["candidates"], g.knn_exact_rows()) == (c0, e0)
    ms = g.last_timing()["phase_ms"]
    assert g.grow(more)[0] == more
    n1, _, samples1 = g.sizes()
    c1, e1 = knn_rows(g.roadmap()[0], n0, n1, samples1, k)
    print("knn candidates", c0, c1, "exact rows", e0, e1)
    assert e0 > 0 and e1 > 0                                                     # (the scene, by the count above: both calls add rows)
    assert (g.last_timing()["candidates"], g.knn_exact_rows()) == (c0 + c1, e0 + e1)   # construction's plus growth's
    assert bits(g.last_timing()["phase_ms"]) == bits(ms)
    g.close()
