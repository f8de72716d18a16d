"""Filter shapes and life scripts of a PRM handle ("Tests"), shared by tests/test_prm_lifecycle_model.py (CPU:
the counts and conditions claimed here hold in the model) and tests/test_gpu_prm_lifecycle.py (GPU: the device replays them and is
compared with the model bit for bit).  Pure Python + numpy on tests/prm_lifecycle_model.py; nothing is cached in a file.

A FILTER SHAPE is one planted roadmap plus one grow, made so that prm_grow_filter_kernel sees a chosen number of candidates of
which a chosen set is dead: q0, the first sample of stream `stream`, is where the grow's first milestone lands; `c` old milestones
stand on a ring of radius 0.5 r around q0 (every one a candidate), FAR more on a ring of radius 3 r (none a candidate); balls
(cones in SO(3)) that do not contain q0 cover an arc of the near ring and kill what stands there (arc_cover); the arc's ends lie
half-way between two ring milestones.  The old milestones are joined in a chain, re-checked by the model before it is planted.

A SCRIPT is a list of steps, run on a HostRoadmap by run_script(); the trace holds every step's resolved arguments, the model's
return values and the roadmap after it, which is what the GPU test replays and compares."""
import math
import os
import sys

import numpy as np

from prm_lifecycle_model import HostRoadmap, Refusal

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden as mg  # noqa: E402
import make_golden_prm as mp  # noqa: E402
import make_golden_prm_so3 as mp3  # noqa: E402

SEED, FRACTION = 20261021, 0.05
SO3_UNBOUNDED = [0.0, 0.0, 0.0, 1.0, math.pi]   # the handle's bounds; the model's are None (the same space)
NOTHING = dict(spheres=[([-50.0, -50.0], 0.1)], boxes=[])   # a scene that covers no state of the box: one ball far outside it
FAR = 40                                         # old milestones of a filter shape that are no candidates


def spec(kind, dim, radius, max_milestones, stream, knn_k=0):
    return dict(kind=kind, dim=dim, radius=radius, max_milestones=max_milestones, stream=stream, knn_k=knn_k)


def model_of(sp, obstacles, max_milestones=None):
    return HostRoadmap(sp["kind"], sp["dim"], None if sp["kind"] == "so3" else [(0.0, 10.0)] * sp["dim"], sp["radius"],
                       max_milestones or sp["max_milestones"], knn_k=sp["knn_k"], lvs_fraction=FRACTION, seed=SEED, stream=sp["stream"],
                       spheres=obstacles["spheres"], boxes=obstacles["boxes"])


def chain_rows(n):
    return [[v for v in (i - 1, i + 1) if 0 <= v < n] for i in range(n)]


def csr_of(rows):
    offsets = np.zeros(len(rows) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
    return offsets, np.array([v for r in rows for v in r], dtype=np.uint32)


# ---------------------------------------------------------------------------------------------------------------- filter shapes
def _frame(q0):
    """two unit quaternions orthogonal to q0 and to each other (Gram-Schmidt on the axes least aligned with q0)"""
    out = []
    for k in np.argsort(np.abs(q0)):
        v = np.zeros(4)
        v[k] = 1.0
        for u in [np.asarray(q0)] + out:
            v = v - (v @ u) * u
        out.append(v / np.linalg.norm(v))
        if len(out) == 2:
            return out


def ring_point(kind, q0, a, phi):
    """the state at distance a from q0 in the direction phi of a fixed plane through q0"""
    if kind == "so3":
        u1, u2 = _frame(q0)
        q = math.cos(a) * np.asarray(q0) + math.sin(a) * (math.cos(phi) * u1 + math.sin(phi) * u2)
        return [float(v) for v in q / np.linalg.norm(q)]
    return [q0[0] + a * math.cos(phi), q0[1] + a * math.sin(phi)]


def arc_cover(kind, q0, a, lo, hi):
    """balls whose union covers exactly the arc [lo, hi] of the ring of radius a around q0.  Their centres stand at distance 2 a from
    q0 and their radius is just below sqrt(3) a, so none contains q0, and where a ball's edge crosses the ring the straight line from q0
    to the ring is nearest to the ball at its far end: a milestone next to the arc can still be reached from q0."""
    big, rho = 2.0 * a, 0.99 * math.sqrt(3.0) * a
    if kind == "so3":
        w = math.acos((math.cos(rho) - math.cos(a) * math.cos(big)) / (math.sin(a) * math.sin(big)))
    else:
        w = math.acos((a * a + big * big - rho * rho) / (2.0 * a * big))
    assert hi - lo >= 2.0 * w, "an arc shorter than one ball"
    k = max(2, int(math.ceil((hi - lo) / (2.0 * w * 0.98))))
    return [(ring_point(kind, q0, big, phi), rho) for phi in np.linspace(lo + w, hi - w, k)]


def stream_for(sp, base):
    """the first stream id >= base whose first sample leaves room for both rings inside the box (any stream in SO(3))"""
    while True:
        q0 = model_of(sp, dict(spheres=[], boxes=[])).sample(mg.ChaCha12Rng(SEED, base))
        if sp["kind"] == "so3" or all(3.5 * sp["radius"] <= v <= 10.0 - 3.5 * sp["radius"] for v in q0):
            return base, q0
        base += 1


def rechecked_chain(sp, obstacles, states):
    """the chain 0 - 1 - ... - n-1 over `states` after the model's own re-check under `obstacles`: rows a re-check leaves alone"""
    m = model_of(sp, obstacles)
    m.plant(states, *csr_of(chain_rows(len(states))))
    m.revalidate()
    return m.csr()


def ring_shape(name, kind, c, dead, stream, far_dead=0, radius=None, what=""):
    """dead: the ring indices [first, first + count) (mod c) that an arc covers, or None"""
    r = radius or (0.3 if kind == "so3" else 0.4)
    sp = spec(kind, 4 if kind == "so3" else 2, r, c + FAR, 0)
    stream, q0 = stream_for(sp, stream)
    step = 2.0 * math.pi / c
    states = [ring_point(kind, q0, 0.5 * r, i * step) for i in range(c)] + [ring_point(kind, q0, 3.0 * r, 0.3 + i * 2.0 * math.pi / FAR) for i in range(FAR)]
    balls = []
    if dead is not None:
        first, count = dead
        balls += arc_cover(kind, q0, 0.5 * r, (first - 0.5) * step, (first + count - 0.5) * step)
    balls += [(states[c + i], 0.02 * r) for i in range(far_dead)]
    offsets, nbrs = rechecked_chain(sp, dict(spheres=balls, boxes=[]), states)
    return dict(name=name, spec=sp, obstacles=dict(spheres=balls, boxes=[]), states=np.array(states), offsets=offsets, nbrs=nbrs, n_more=1,
                stream=stream, q0=q0, ring=c, ring_dead=0 if dead is None else dead[1], far_dead=far_dead, candidates=c, what=what)


def new_new_shape():
    """65 new milestones under a radius that spans the box, every old milestone under one ball: all 65 n_old old-new candidates go,
    the 65 * 64 / 2 new-new ones stay"""
    c, r, stream, centre = 64, 15.0, 41, [2.0, 2.0]
    sp = spec("rn", 2, r, c + FAR, 0)
    states = [ring_point("rn", centre, 0.5, i * 2.0 * math.pi / c) for i in range(c)] + [ring_point("rn", centre, 0.8, 0.3 + i * 2.0 * math.pi / FAR) for i in range(FAR)]
    offsets, nbrs = rechecked_chain(sp, dict(spheres=[(centre, 1.0)], boxes=[]), states)
    return dict(name="new_new_only", spec=sp, obstacles=dict(spheres=[(centre, 1.0)], boxes=[]), states=np.array(states), offsets=offsets, nbrs=nbrs,
                n_more=65, stream=stream, q0=None, ring=c, ring_dead=c, far_dead=FAR, candidates=65 * (c + FAR) + 65 * 64 // 2,
                what="every surviving pair has i >= n_old")


EDGE_C = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023]


def _shapes():
    out = {}
    for k, c in enumerate(EDGE_C):   # about half of the ring under one arc (of a ring of one: the one)
        out["edge_%d" % c] = lambda c=c, k=k: ring_shape("edge_%d" % c, "rn", c, (0, (c + 1) // 2), 20 + k, what="compaction offsets at wave and workgroup edges")
    for c in (64, 257):
        out["all_dropped_%d" % c] = lambda c=c: ring_shape("all_dropped_%d" % c, "rn", c, (0, c), 33, what="*count stays 0: an empty new row, the old CSR after the re-sort")
    out["identity_257"] = lambda: ring_shape("identity_257", "rn", 257, None, 34, far_dead=3, what="the filter runs and drops nothing")
    for label, k in (("first", 0), ("63", 63), ("last", 256)):
        out["one_kept_%s" % label] = lambda k=k, label=label: ring_shape("one_kept_%s" % label, "rn", 257, (k + 1, 256), 35, what="a single survivor wherever it falls")
    out["new_new_only"] = new_new_shape
    out["so3_edge_65"] = lambda: ring_shape("so3_edge_65", "so3", 65, (0, 33), 36, what="the same kernel on SO(3)'s candidates")
    out["so3_all_dropped"] = lambda: ring_shape("so3_all_dropped", "so3", 65, (0, 65), 37, what="SO(3): *count stays 0")
    return out


SHAPES = _shapes()
_SHAPE, _GROWN = {}, {}


def shape(name):
    if name not in _SHAPE:
        _SHAPE[name] = SHAPES[name]()
        for k in ("states", "offsets", "nbrs"):
            _SHAPE[name][k].setflags(write=False)
    return _SHAPE[name]


def planted_model(sh, obstacles=None):
    m = model_of(sh["spec"], sh["obstacles"] if obstacles is None else obstacles)
    m.plant(sh["states"], sh["offsets"], sh["nbrs"])
    return m


def grown(name):
    """the model after the shape's one grow, made once per process: dict(model, added, drawn, live, valid_after, removed_after)"""
    if name not in _GROWN:
        sh = shape(name)
        m = planted_model(sh)
        live = np.array([m.is_valid(s) for s in m.states], dtype=bool)
        added, drawn = m.grow(sh["n_more"], new_stream=sh["stream"])
        rm, sizes = m.roadmap(), m.sizes()
        valid, removed = m.revalidate()
        _GROWN[name] = dict(model=m, added=added, drawn=drawn, live=live, roadmap=rm, sizes=sizes, valid_after=valid, removed_after=removed)
    return _GROWN[name]


def candidate_count(sh, states):
    """the pairs (j, i), j a milestone of the call, i < j, with distance < r"""
    m = model_of(sh["spec"], sh["obstacles"])
    n_old = len(sh["states"])
    return sum(1 for j in range(n_old, len(states)) for i in range(j) if m.distance(states[j], states[i]) < sh["spec"]["radius"])


# ---------------------------------------------------------------------------------------------------------------- scenes
def _pocket(lo, hi, t, dim):
    """thin boxes of thickness t that wall in the cube [lo, hi]^dim: what lies inside is a component of its own"""
    out = []
    for k in range(dim):
        for side in (lo - t, hi):
            a, b = [lo - t] * dim, [hi + t] * dim
            a[k], b[k] = side, side + t
            out.append((a, b))
    return out


def _unit(q):
    q = np.asarray(q, dtype=np.float64)
    return (q / np.linalg.norm(q)).tolist()


# scene A, and what scene B adds: a large obstacle that covers milestones and thin ones that only cut edges
SCENES = {
    "r2": dict(A=dict(spheres=[([3.0, 3.0], 1.0), ([7.0, 6.0], 0.8)], boxes=[([4.5, 7.0], [6.0, 8.5])] + _pocket(0.8, 2.0, 0.2, 2)),
               B=dict(spheres=[([5.0, 2.0], 1.2), ([1.5, 7.5], 0.15), ([8.0, 2.5], 0.15)], boxes=[([6.5, 8.8], [9.5, 8.9]), ([0.3, 5.0], [4.2, 5.08]), ([8.5, 3.0], [8.58, 7.5])])),
    "r3": dict(A=dict(spheres=[([3.0, 3.0, 3.0], 1.2), ([7.0, 6.0, 5.0], 1.0), ([2.0, 8.0, 6.0], 0.9)],
                      boxes=[([4.5, 7.0, 1.0], [6.0, 8.5, 3.0])] + _pocket(7.0, 9.0, 0.2, 3)),
               B=dict(spheres=[([5.0, 5.0, 5.5], 2.0), ([2.0, 6.0, 2.0], 0.6), ([8.0, 2.0, 7.0], 0.6), ([6.5, 1.5, 4.0], 0.6), ([1.5, 2.0, 8.0], 0.6)],
                      boxes=[])),
    "so3": dict(A=dict(spheres=[(_unit([1, 0, 0, 1]), 0.35), (_unit([0, 1, 1, 0]), 0.3)], boxes=[]),
                B=dict(spheres=[(_unit([0, 0, 1, 1]), 0.5), (_unit([1, 1, 1, 1]), 0.15), (_unit([1, -1, 0, 2]), 0.15), (_unit([0, 2, -1, 1]), 0.15),
                                (_unit([3, 0, 1, -1]), 0.15),
                                # four thin cones on edges of so3_life's first 300 milestones: they cut an edge and cover neither end
                                (_unit([0.236, 0.0765, 0.389, -0.8872]), 0.04), (_unit([-0.4235, 0.5401, 0.1266, 0.7162]), 0.04),
                                (_unit([-0.8413, 0.4169, -0.2281, -0.2577]), 0.04), (_unit([-0.6633, 0.1326, 0.6552, 0.3363]), 0.04)], boxes=[])),
}


def scene(name, which):
    a, b = SCENES[name]["A"], SCENES[name]["B"]
    if which == "A":
        return dict(spheres=list(a["spheres"]), boxes=list(a["boxes"]))
    return dict(spheres=a["spheres"] + b["spheres"], boxes=a["boxes"] + b["boxes"])


# ---------------------------------------------------------------------------------------------------------------- scripts
# A step is (op, arguments).  grow: n_more or to (the milestone count to reach), new_stream, cap = "stays" (lands exactly on the
# capacity) / "moves" (crosses it), refused = (status name, text fragment).  prune: invalid, mask ("every_second"), min_size,
# largest.  fresh: the roadmap equals a fresh handle's construction to n milestones.
def S(op, **kw):
    return (op, kw)


SCRIPTS = {
    "refill": dict(spec=spec("rn", 2, 0.5, 300, 3), scene="r2", start="A", steps=[
        S("construct"), S("scene", which="B"), S("revalidate"), S("grow", n_more=100), S("prune", invalid=True), S("grow", to=1024, cap="stays"),
        S("grow", n_more=1, cap="moves"), S("scene", which="A"), S("revalidate"), S("components"), S("prune", largest=True), S("grow", n_more=50),
        S("grow", to=2049, cap="moves")]),
    "planted_veteran": dict(spec=spec("rn", 3, 1.5, 900, 3), scene="r3", start="B", steps=[
        S("plant", built_in="A"), S("grow", n_more=124, new_stream=7, cap="stays"), S("grow", n_more=1, cap="moves"),
        S("prune", mask="every_second", min_size=2), S("grow", n_more=30), S("revalidate"), S("prune", invalid=True, largest=True)]),
    "odd_capacity": dict(spec=spec("rn", 2, 0.3, 2049, 5), scene="r2", start="A", steps=[
        S("construct"), S("scene", which="B"), S("revalidate"), S("grow", to=3072, cap="stays"), S("grow", n_more=1, cap="moves"), S("components"),
        S("prune", min_size=3)]),
    "knn_life": dict(spec=spec("knn", 3, 1.5, 200, 3, knn_k=5), scene="r3", start="A", steps=[
        S("construct"), S("scene", which="B"), S("grow", n_more=10, refused=("BAD_ARG", "not built")), S("prune", invalid=True),
        S("grow", to=1025, cap="moves"), S("components"), S("prune", largest=True), S("grow", n_more=40), S("revalidate")]),
    "setup_again": dict(spec=spec("rn", 2, 0.5, 300, 3), scene="r2", start="A", steps=[
        S("construct"), S("grow", n_more=800, cap="moves"), S("setup"), S("construct"), S("fresh", n=300), S("grow", n_more=10), S("fresh", n=310)]),
    "so3_life": dict(spec=spec("so3", 4, 0.25, 300, 3), scene="so3", start="A", steps=[
        S("construct"), S("scene", which="B"), S("revalidate"), S("grow", n_more=100), S("prune", invalid=True), S("grow", to=1025, cap="moves"),
        S("components"), S("prune", largest=True)]),
}
_TRACE = {}


def keep_mask(name, n):
    assert name == "every_second"
    return np.arange(n) % 2 == 0


def run_script(name):
    """the script on the model, once per process: a list with one record per step -- op, args (resolved: a grow has n_more), result (the
    model's return values, or the Refusal), roadmap / sizes / capacity after it, cap_before, obstacles (as they are now), changed
    (the roadmap may differ from the step before), marked (the full twin check runs after it)"""
    if name in _TRACE:
        return _TRACE[name]
    sc = SCRIPTS[name]
    obstacles = scene(sc["scene"], sc["start"])
    m = model_of(sc["spec"], obstacles)
    trace = []
    for k, (op, kw) in enumerate(sc["steps"]):
        args, result, cap_before, n_before = dict(kw), None, m.capacity, m.n
        if op == "construct":
            m.construct()
        elif op == "setup":
            m.setup()
        elif op == "scene":
            obstacles = scene(sc["scene"], kw["which"])
            m.set_obstacles(**obstacles)
        elif op == "plant":
            src = model_of(sc["spec"], scene(sc["scene"], kw["built_in"]))
            src.construct()
            args["roadmap"] = src.roadmap()
            m.plant(*args["roadmap"])
        elif op == "revalidate":
            result = m.revalidate()
        elif op == "grow":
            if "to" in kw:
                args["n_more"] = kw["to"] - m.n
            try:
                result = m.grow(args["n_more"], new_stream=kw.get("new_stream"))
            except Refusal as e:
                result = e
        elif op == "prune":
            if "mask" in kw:
                args["keep"] = keep_mask(kw["mask"], m.n)
            result = m.prune(invalid=kw.get("invalid", False), keep=args.get("keep"), min_size=kw.get("min_size", 0), largest=kw.get("largest", False))
        elif op == "components":
            result = m.components()
        elif op == "fresh":
            f = model_of(sc["spec"], obstacles, max_milestones=kw["n"])
            f.construct()
            result = (f.roadmap(), f.sizes())
        else:
            raise AssertionError(op)
        changed = op in ("construct", "plant", "revalidate", "grow", "prune") and not isinstance(result, Refusal)
        marked = changed and (op == "prune" or m.capacity != cap_before or k == len(sc["steps"]) - 1) and m.n > 0
        trace.append(dict(op=op, args=args, result=result, roadmap=m.roadmap(), sizes=m.sizes(), capacity=m.capacity, cap_before=cap_before,
                          n_before=n_before, obstacles=obstacles, changed=changed, marked=marked))
    last = [t for t in trace if t["changed"]][-1]
    last["marked"] = True
    _TRACE[name] = trace
    return trace


# ---------------------------------------------------------------------------------------------------------------- queries of the twin check
def queries(sp, count, seed):
    """(starts, goals, goal radii): short queries anywhere in the space, so that sparse roadmaps answer some of them too"""
    rng = np.random.default_rng(seed)
    if sp["kind"] == "so3":
        s = rng.normal(size=(count, 4))
        s /= np.linalg.norm(s, axis=1, keepdims=True)
        g = s + 0.3 * rng.normal(size=(count, 4))
        g /= np.linalg.norm(g, axis=1, keepdims=True)
        return s, g, np.full(count, 0.3)
    s = rng.uniform(0.5, 9.5, size=(count, sp["dim"]))
    g = np.clip(s + rng.uniform(-1.0, 1.0, size=s.shape), 0.2, 9.8)
    return s, g, np.full(count, max(1.5 * sp["radius"], 0.6))


def model_solve(sp, obstacles, roadmap, start, goal, goal_r):
    """(status, path) of one query on `roadmap` by the golden generators' prm_solve: "solved" / "no_solution" / "invalid_start" """
    states, offsets, nbrs = roadmap
    m = model_of(sp, obstacles)
    edges = [[int(v) for v in nbrs[int(offsets[i]):int(offsets[i + 1])]] for i in range(len(states))]
    start, goal = [float(v) for v in start], [float(v) for v in goal]
    if sp["kind"] == "so3":
        st, _, _, path = mp3.prm_solve(sp["radius"], FRACTION, m.field, dict(states=[[float(v) for v in r] for r in states], edges=edges), start, goal, goal_r)
    else:
        st, _, _, path = mp.prm_solve(sp["dim"], m.bounds, sp["radius"], FRACTION, m.field, dict(states=np.asarray(states), edges=edges), start, goal, goal_r)
    return st, np.array(path, dtype=np.float64).reshape(len(path), sp["dim"])
