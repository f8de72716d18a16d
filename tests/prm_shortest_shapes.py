"""Scenes for the shortest-path PRM batch that the three recorded ones -- compact blobs in general position --
cannot stand for: roadmaps on a line, where collinear distances add up to equal sums bit for bit and distance weights meet the
tie rule; long thin roadmaps with deep levels; mean degrees for each of the five lane groups; roadmaps with isolated milestones;
and the dimensions no other PRM test uses.  No obstacles anywhere, so no start is invalid and the shapes come from geometry alone.

Each row of SCENES is a parameter dict in the shape make_gpu_prm (prm_shortest_helpers.py) and gp.prm_construct take.  GROUP and
the conditions of tests/test_prm_shortest_shapes_model.py are what the GPU test relies on; that test holds them on the CPU, from
the pure-Python generators, which build the device's roadmap bit for bit."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden as mg  # noqa: E402
import make_golden_prm as gp  # noqa: E402
import make_golden_prm_shortest as gsp  # noqa: E402

QUERY_SEED = 20261101


def _scene(bounds, radius, milestones, query_stream):
    """query_stream: the scene's own stream of the query generator, fixed here so that a new scene changes no other scene's queries"""
    return dict(dim=len(bounds), bounds=[tuple(b) for b in bounds], radius=radius, fraction=0.05, spheres=[], boxes=[], seed=7, stream=1,
                max_milestones=milestones, max_samples=10 ** 9, query_stream=query_stream)


SQUARE = [(0.0, 10.0)] * 2
SCENES = {
    "line": _scene([(0.0, 64.0)], 1.0, 400, 3),
    "line_dense": _scene([(0.0, 64.0)], 3.0, 400, 4),
    "strip": _scene([(0.0, 64.0), (0.0, 0.001)], 1.0, 400, 11),
    "sparse": _scene(SQUARE, 0.6, 300, 10),
    "dust": _scene(SQUARE, 0.35, 300, 0),
    "g8": _scene(SQUARE, 0.85, 300, 2),
    "g32": _scene(SQUARE, 1.0, 600, 1),
    "r3": _scene([(0.0, 10.0)] * 3, 2.5, 256, 5),
    "r4": _scene([(0.0, 10.0)] * 4, 3.5, 256, 6),
    "r5": _scene([(0.0, 10.0)] * 5, 4.5, 256, 7),
    "r7": _scene([(0.0, 10.0)] * 7, 6.0, 256, 8),
    "r8": _scene([(0.0, 10.0)] * 8, 7.0, 256, 9),
}
LONG = ("line", "line_dense", "strip")
# lanes per node (prm_batch_group) that each scene's roadmap selects: all five between them
GROUP = {"line": 16, "line_dense": 64, "strip": 16, "sparse": 4, "dust": 4, "g8": 8, "g32": 32, "r3": 16, "r4": 16, "r5": 16, "r7": 16,
         "r8": 16}
ALL_LABELS = ("line", "line_dense", "strip", "sparse")       # scenes whose every label, hops and parent the GPU test compares


def n_queries(name):
    return 64 if name in LONG else 32


def goal_radii(name):
    """the range of goal radii: a ball that holds a few milestones at the scene's density"""
    P = SCENES[name]
    if name in LONG:
        return 0.5, 2.0
    if P["dim"] == 2:
        return 0.3, 0.8
    return 0.5 * P["radius"], 0.8 * P["radius"]


def queries(name, n=None):
    """-> (starts [n][dim], goal centres [n][dim], goal radii [n]) as lists of floats: uniform in the bounds / in goal_radii(name)"""
    P = SCENES[name]
    n = n_queries(name) if n is None else n
    rng = np.random.default_rng([QUERY_SEED, P["query_stream"]])
    lo = np.array([b[0] for b in P["bounds"]])
    hi = np.array([b[1] for b in P["bounds"]])
    starts = rng.uniform(lo, hi, size=(n, P["dim"]))
    goals = rng.uniform(lo, hi, size=(n, P["dim"]))
    radii = rng.uniform(*goal_radii(name), size=n)
    return starts.tolist(), goals.tolist(), [float(v) for v in radii]


def batch_group(n, n_edge_entries):
    """prm_batch_group (prm_batch.hip): the least of 4, 8, 16, 32, 64 that is no less than the mean degree, rounded up"""
    mean = (n_edge_entries + n - 1) // n if n else 0
    g = 4
    while g < 64 and g < mean:
        g <<= 1
    return g


def library_group(n, n_edge_entries):
    """the library's own oxhip::prm_batch_group(uint32_t, uint64_t), which the host code calls before every search launch: an
    internal function, not part of the C ABI, reached by its mangled name because no getter hands the group out.  GPU tests only
    (the library is loaded there already); a change of its signature or visibility shows as an AttributeError here: update the name"""
    import ctypes as C
    from oxmpl_amd import capi
    f = getattr(capi.lib(), "_ZN5oxhip15prm_batch_groupEjm")
    f.argtypes, f.restype = [C.c_uint32, C.c_uint64], C.c_uint32
    return int(f(n, n_edge_entries))


def multi_tight(edges, W, res):
    """cnt[v] = the number of v's tight predecessors one level up, for a checker result `res` (0 for sources and unreached nodes)"""
    c, hops = res["c"], res["hops"]
    cnt = [0] * len(edges)
    for u, lst in enumerate(edges):
        if hops[u] == gsp.UNSET:
            continue
        cu, hu, wu = c[u], hops[u] + 1, W[u]
        for k, v in enumerate(lst):
            if hops[v] == hu and cu + wu[k] == c[v]:
                cnt[v] += 1
    return cnt


_models = {}


def model(name):
    """The scene on the CPU, from the pure-Python generators alone: the roadmap, and its queries answered in distance mode.
    -> dict(n, entries, group, mean_degree, isolated, statuses (prm_solve's), results (shortest_query's), solved, multi_tight,
    chain_ties (solved queries whose answer passes through a node with two or more tight predecessors), max_hops, deepest (the
    query that has them), demoted (start connections with c[m] < init[m]), invalid_starts)"""
    if name in _models:
        return _models[name]
    P = SCENES[name]
    field = mg.Field(P["dim"])
    rm = gp.prm_construct(P["dim"], P["bounds"], P["radius"], P["fraction"], field, P["seed"], P["stream"], P["max_milestones"],
                          P["max_samples"])
    edges, states = rm["edges"], rm["states"]
    n, entries = len(edges), sum(len(lst) for lst in edges)
    W = gsp.edge_weights(edges, states, mg.distance, gsp.DISTANCE)
    out = dict(n=n, entries=entries, group=batch_group(n, entries), mean_degree=entries / n, isolated=sum(not lst for lst in edges),
               statuses=[], results=[], solved=0, multi_tight=0, chain_ties=0, max_hops=0, deepest=0, demoted=0, invalid_starts=0)
    for q, (start, goal_c, goal_r) in enumerate(zip(*queries(name))):
        status, sc, gi, _ = gp.prm_solve(P["dim"], P["bounds"], P["radius"], P["fraction"], field, rm, start, goal_c, goal_r)
        out["statuses"].append(status)
        out["invalid_starts"] += status == "invalid_start"
        init = gsp.init_labels(n, sc, start, states, mg.distance, gsp.DISTANCE)
        res = gsp.shortest_query(edges, W, init, gi)
        assert res["status"] == status, (name, q)
        out["results"].append(res)
        cnt = multi_tight(edges, W, res)
        out["multi_tight"] += sum(k >= 2 for k in cnt)
        out["demoted"] += sum(res["c"][m] < init[m] for m in sc)
        deepest = max((h for h in res["hops"] if h != gsp.UNSET), default=0)
        if deepest > out["max_hops"]:
            out["max_hops"], out["deepest"] = deepest, q
        if status == "solved":
            out["solved"] += 1
            out["chain_ties"] += any(cnt[v] >= 2 for v in res["nodes"])
    _models[name] = out
    return out
