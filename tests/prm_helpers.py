"""Test-side helpers for the PRM parity tests (may use the oracle)."""
import numpy as np

from helpers import bits, params_spheres, params_boxes

FNV_P = 0x100000001B3
MASK = (1 << 64) - 1
STATUS_NAME = {0: "solved", 1: "timeout", 2: "no_solution", 3: "uninitialised", 4: "invalid_start", 5: "unsampled"}


def csr_checksum(offsets, nbrs):
    """FNV-1a over (degree, neighbours...) per node, as tests/golden/make_golden_prm.py"""
    h = 0xCBF29CE484222325
    for i in range(len(offsets) - 1):
        a, b = int(offsets[i]), int(offsets[i + 1])
        h = ((h ^ (b - a)) * FNV_P) & MASK
        for v in nbrs[a:b]:
            h = ((h ^ int(v)) * FNV_P) & MASK
    return h


def states_checksum(states):
    h = 0xCBF29CE484222325
    for v in np.ascontiguousarray(states, dtype=np.float64).view(np.uint64).ravel():
        h = ((h ^ int(v)) * FNV_P) & MASK
    return h


def make_oracle_prm(P, **kw):
    from oracle import oracle_py as orc
    o = orc.OraclePRM(P["dim"], P["bounds"], P["radius"], lvs_fraction=P["fraction"], seed=P["seed"],
                      stream=P["stream"], **kw)
    if P["spheres"]:
        c, r = params_spheres(P)
        o.set_spheres(c, r)
    if P["boxes"]:
        lo, hi = params_boxes(P)
        o.set_boxes(lo, hi)
    if P.get("knn_k"):
        o.set_knn(P["knn_k"])
    return o


def make_gpu_prm(P, **kw):
    from oxmpl_amd import capi
    args = dict(max_milestones=P["max_milestones"], lvs_fraction=P["fraction"], seed=P["seed"], stream=P["stream"],
                max_samples=0 if P["max_samples"] >= 10 ** 9 else P["max_samples"])
    args.update(kw)
    g = capi.PRMRoadmap(P["dim"], P["bounds"], P["radius"], **args)
    if P["spheres"]:
        g.set_spheres(*params_spheres(P))
    if P["boxes"]:
        g.set_boxes(*params_boxes(P))
    return g


def assert_same_roadmap(g, o):
    n, e, s = g.sizes()
    assert n == o.num_milestones and s == o.num_samples
    gs, goff, gn = g.roadmap()
    os_, ooff, on = o.roadmap()
    assert np.array_equal(bits(gs), bits(os_))
    assert np.array_equal(goff, ooff)
    assert np.array_equal(gn, on)
    return gs, goff, gn


def assert_same_query(g, o, timeout=0.0):
    from oxmpl_amd import capi
    st, path = g.solve(timeout)
    ost = o.solve()
    assert st == ost
    if st not in (capi.ERR_INVALID_START_STATE, capi.ERR_UNSAMPLED_STATE_SPACE, capi.ERR_PLANNER_UNINITIALISED):
        sc, gi = g.query_sets()
        assert np.array_equal(sc, o.start_connections())
        assert np.array_equal(gi, o.goal_indices())
    opath = o.path()
    assert path.shape == opath.shape and np.array_equal(bits(path), bits(opath))
    return st, path
