"""Scenes for RRT* (planner kind 2: rrt_star_wire.hip's six kernels behind wire_new_nodes, and rrt_star.hip) at the limits the golden
scenes do not reach, and an instrumented replay that says what a scene holds.
  slab    R^1 .. R^8 with 2-D density (every further axis is 1/16 wide), 100 spheres -- more than one 64-sphere chunk of star_edges --
          and a box: hundreds of rewires, changed parents and obstacle-rejected neighbour motions in EVERY dimension
  reach   every sample inserted where it falls and half the samples bit-equal copies of the goal: thousands of exact cost ties in
          choose-parent and in rewiring, lists longer than 64 entries, minima shared between 64-entry blocks
  mixed   10 problems of one batch with goal radii from 100 (ends at its first node) through 0 (ends at a bit-equal copy of the goal) to
          -1 (runs to the node cap), search radius +inf
  frames  the R^5 slab translated by 1e6, scaled by 1e40 and by 1e-12
  large   a 33,000-node tree in R^2: node indices beyond 2^15

Constructions only: nothing here loads the GPU library.  The replay restates oxmpl's RRTStar::solve on the primitives of
tests/golden/make_golden.py in the order of tests/golden/make_golden_rrt_star.py (rrt_star.rs:170-289) and counts; that it and the C
oracle (oracle/rrt_oracle.c) agree bit for bit, and that every scene holds what tests/test_gpu_rrt_star_limits.py relies on, is held
on the CPU by tests/test_rrt_star_limits_model.py.  Replays and oracle runs are computed once (functools caches) and shared: never
modify one."""
import functools
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden as mg  # noqa: E402
from make_golden_rrt_star import FNV_P, M64, row_dists  # noqa: E402

from helpers import params_boxes, params_spheres  # noqa: E402

FRACTION = 0.05
SEED = 7
PIDS = (3, 4, 5)                 # pid 3 is the replayed one; the GPU test runs all three
BUDGET = 10 ** 6                 # iterations: every scene ends at its node cap (or its goal) long before
BLOCK = 64                       # star_wire takes a neighbour list 64 entries at a time; star_edges the spheres 64 at a time
INF = math.inf


# ----------------------------------------------------------------------------------------------------------------- scenes
def _scene(dim, bounds, max_distance, goal_bias, search_radius, start, goal_c, goal_r, spheres, boxes, max_nodes):
    return dict(dim=dim, bounds=[(float(lo), float(hi)) for lo, hi in bounds], max_distance=max_distance, goal_bias=goal_bias,
                search_radius=search_radius, fraction=FRACTION, start=[float(v) for v in start], goal_c=[float(v) for v in goal_c],
                goal_r=goal_r, spheres=spheres, boxes=boxes, max_nodes=max_nodes)


def _slab_frame(dim):
    bounds = ([(0.0, 10.0), (0.0, 10.0)] + [(5.0, 5.0625)] * 6)[:dim]
    start = ([1.0, 1.0] + [5.03125] * 6)[:dim]
    goal = ([9.0, 9.0] + [5.03125] * 6)[:dim]
    return bounds, start, goal


@functools.lru_cache(maxsize=None)
def slab_scene(dim):
    """2-D density in a dim-dimensional instantiation (R^1: the plain line, which the box then cuts at 4)"""
    bounds, start, goal = _slab_frame(dim)
    rng = np.random.default_rng(100 + dim)
    centres = rng.uniform([lo for lo, _ in bounds], [hi for _, hi in bounds], size=(100, dim))
    radii = rng.uniform(0.15, 0.5, size=100)
    spheres = [([float(v) for v in c], float(r)) for c, r in zip(centres, radii)
               if all(mg.distance(list(c), p) > r + 0.3 for p in (start, goal))]
    box = (([4.0, 0.0] + [0.0] * 6)[:dim], ([4.4, 4.6] + [10.0] * 6)[:dim])
    return _scene(dim, bounds, 0.5, 0.05, 1.0, start, goal, 0.3, spheres, [box], 600)


REACH_VARIANTS = ("free", "box")


@functools.lru_cache(maxsize=None)
def reach_scene(dim, variant):
    """max_distance 100: q_new = q_rand; goal bias 0.5: half the nodes are the goal centre, bit for bit"""
    boxes = [([3.0] * dim, [4.0] * dim)] if variant == "box" else []
    return _scene(dim, [(0.0, 10.0)] * dim, 100.0, 0.5, 3.0 if dim <= 3 else 5.0, [1.0] * dim, [6.0] * dim, 0.3, [], boxes, 300)


# radius 100 ends a problem at its first inserted node; radius 0 only at a bit-equal copy of the goal centre (distance <= 0: a goal
# sample drawn when the tree is within max_distance of it); a negative radius never, so that problem runs to the node cap
MIXED_RADII = (100.0, 100.0, 3.0, 1.0, 0.5, 0.25, 0.0, 0.0, -1.0, -1.0)
# run -> (max_nodes, the budgets of its solve calls).  two_calls: the capped problems bring more than 100,000 neighbour entries to the
# second call.  A round of wire_new_nodes takes at most a pool segment of entries (64 per node of capacity, the capacity a multiple
# of 1024), so at 500 nodes no round reaches the 65,536 entries from which the edge checks are cut into eight segments; one_call's
# first round does, next to the problems that ended at their first node and bring ONE entry to it.
MIXED_RUNS = {"two_calls": (500, (60, BUDGET)), "one_call": (1100, (BUDGET,))}
POOL_PER_NODE, CAP_QUANTUM, EIGHT_SEGMENTS_FROM = 64, 1024, 64 * 1024


@functools.lru_cache(maxsize=None)
def mixed_scene(dim, run):
    """the slab world without obstacles, every node a neighbour of every later one; goal_r is per problem"""
    bounds, start, goal = _slab_frame(dim)
    return _scene(dim, bounds, 0.5, 0.05, INF, start, goal, list(MIXED_RADII), [], [], MIXED_RUNS[run][0])


def problem_scene(P, p):
    """problem p of a batch whose problems have their own goal radius"""
    return dict(P, goal_r=P["goal_r"][p])


@functools.lru_cache(maxsize=None)
def mixed_geometry(dim, run, p, iterations):
    """(nodes, goal node) of problem p after `iterations`: an RRT* run's node positions, node count and goal node are RRT's on the same
    stream (no cost enters them), so make_golden.rrt_solve says them"""
    P = problem_scene(mixed_scene(dim, run), p)
    res = mg.rrt_solve(dim, P["bounds"], P["max_distance"], P["goal_bias"], FRACTION, mg.Field(dim), P["start"], P["goal_c"], P["goal_r"],
                       SEED, PIDS[0] + p, iterations, P["max_nodes"], stop_at_goal=True)
    return res["n"], res["goal_node"]


def entries_between(n0, n1):
    """neighbour entries of the nodes [n0, n1) at search radius +inf: node i's list is 0 .. i-1"""
    return n1 * (n1 - 1) // 2 - n0 * (n0 - 1) // 2


def wiring_rounds(n0, n1, max_nodes):
    """the entries of each wiring round of the nodes [n0, n1) at radius +inf: a round takes the longest prefix of the pending nodes
    whose lists fit the pool segment"""
    share = POOL_PER_NODE * ((max_nodes + CAP_QUANTUM - 1) // CAP_QUANTUM * CAP_QUANTUM)
    rounds, total = [], 0
    for i in range(n0, n1):
        if total + i > share:
            rounds.append(total)
            total = 0
        total += i
    return rounds + [total] if total else rounds


FRAMES = {"far": (1.0, 1.0e6), "huge": (1.0e40, 0.0), "tiny": (1.0e-12, 0.0)}   # name -> (scale, offset)
FRAME_DIM = 5
FRAME_PIDS = PIDS[:2]


@functools.lru_cache(maxsize=None)
def frame_scene(frame):
    """the R^5 slab as test_rrt_star_translated_and_scaled_spaces moves a scene: far from the origin binary32 separates nothing,
    beyond 1e15 star_pairs' screen is off, 1e-12 sits at binary32's subnormal end"""
    scale, offset = FRAMES[frame]
    B = slab_scene(FRAME_DIM)
    t = lambda v: [float(x) * scale + offset for x in v]
    c, r = params_spheres(B)
    c, r = c * scale + offset, r * scale
    return dict(B, bounds=[tuple(t(b)) for b in B["bounds"]], start=t(B["start"]), goal_c=t(B["goal_c"]),
                max_distance=B["max_distance"] * scale, goal_r=B["goal_r"] * scale, search_radius=B["search_radius"] * scale,
                spheres=[([float(v) for v in row], float(rad)) for row, rad in zip(c, r)], boxes=[(t(lo), t(hi)) for lo, hi in B["boxes"]])


LARGE_SEED, LARGE_PID = 5, 1
HALF_U16 = 1 << 15


@functools.lru_cache(maxsize=None)
def large_scene():
    return _scene(2, [(0.0, 10.0)] * 2, 0.25, 0.05, 0.1, [1.0, 1.0], [9.0, 9.0], 0.3, [([5.0, 5.0], 1.0), ([2.0, 7.0], 0.7)], [], 33000)


# ----------------------------------------------------------------------------------------------------------------- the oracle
def make_oracle(P, seed, pid, stop=False):
    from oracle import oracle_py as orc
    o = orc.OracleRRTStar(P["dim"], P["bounds"], P["max_distance"], P["goal_bias"], P["search_radius"], P["fraction"], P["max_nodes"],
                          stop, seed, pid)
    if P["spheres"]:
        o.set_spheres(*params_spheres(P))
    if P["boxes"]:
        o.set_boxes(*params_boxes(P))
    o.setup(P["start"], P["goal_c"], P["goal_r"])
    return o


def _solved(P, seed, pid, stop=False, iterations=BUDGET):
    o = make_oracle(P, seed, pid, stop)
    o.solve(iterations)
    return o


@functools.lru_cache(maxsize=None)
def slab_oracle(dim, pid):
    return _solved(slab_scene(dim), SEED, pid)


@functools.lru_cache(maxsize=None)
def reach_oracle(dim, variant, pid):
    return _solved(reach_scene(dim, variant), SEED, pid)


@functools.lru_cache(maxsize=None)
def frame_oracle(frame, pid):
    return _solved(frame_scene(frame), SEED, pid)


@functools.lru_cache(maxsize=None)
def large_oracle():
    return _solved(large_scene(), LARGE_SEED, LARGE_PID)


@functools.lru_cache(maxsize=None)
def mixed_oracle(dim, run, p, iterations):
    """problem p after `iterations` in all (the oracle's result does not depend on how the budget is cut)"""
    return _solved(problem_scene(mixed_scene(dim, run), p), SEED, PIDS[0] + p, stop=True, iterations=iterations)


# ----------------------------------------------------------------------------------------------------------------- the replay
def check_motion(field, bounds, fraction, frm, to):
    """make_golden.check_motion with its states as rows: the same binary64 operations in the same order (t = i / n; f + (g - f) * t;
    per sphere the sum over k of (c_k - p_k)^2, sqrt, > r; per box lo <= p <= hi), every state evaluated at once"""
    n = mg.num_steps(mg.distance(frm, to), mg.maximum_extent(bounds) * fraction)
    if n <= 1:
        return field.is_valid(to)
    if n > 100000:
        return mg.check_motion(field, bounds, fraction, frm, to)
    t = np.arange(1, n + 1, dtype=np.float64) / float(n)
    f, g = np.array(frm, dtype=np.float64), np.array(to, dtype=np.float64)
    pts = f[None, :] + (g - f)[None, :] * t[:, None]
    if len(field.sr):
        acc = np.zeros((n, len(field.sr)))
        for k in range(field.dim):
            d = field.sc[None, :, k] - pts[:, k, None]
            acc = acc + d * d
        if not bool(np.all(np.sqrt(acc) > field.sr[None, :])):
            return False
    for lo, hi in field.boxes:
        if bool(np.any(np.all((np.array(lo)[None, :] <= pts) & (pts <= np.array(hi)[None, :]), axis=1))):
            return False
    return True


COUNTERS = ("rewires", "changed_parents", "rejected", "late_only", "parent_ties", "rewire_ties", "shared_minima", "cross_block_minima",
            "long_lists", "longest_list")


def replay(P, seed, pid, max_iterations=BUDGET, stop_at_goal=False):
    """One problem, make_golden_rrt_star.rrt_star_solve's loop with counters (none of them enters the result):
      rewires             parents changed by step 8
      changed_parents     nodes inserted with a parent that is not their nearest node
      rejected            neighbour motions the reference evaluates (its cost test passed) and check_motion refuses
      late_only           ... of them, valid against the first 64 spheres (and the boxes): refused by a sphere of a later chunk alone
      parent_ties         a neighbour other than the running choice with a valid motion and a cost-through EQUAL to the running minimum
      rewire_ties         c2 == cost[j] for a neighbour that is not the parent
      shared_minima       nodes where, among the valid neighbours with a cost-through strictly below the nearest node's route, two or
                          more attain the minimum
      cross_block_minima  ... in different 64-entry blocks of the ascending list
      long_lists / longest_list   lists longer than 64 entries / the longest"""
    dim, bounds, fraction = P["dim"], P["bounds"], P["fraction"]
    max_distance, goal_bias, search_radius, max_nodes = P["max_distance"], P["goal_bias"], P["search_radius"], P["max_nodes"]
    goal_c, goal_r = P["goal_c"], P["goal_r"]
    spheres, boxes = list(zip(*params_spheres(P))) if P["spheres"] else [], P["boxes"]
    field, field64 = mg.Field(dim, spheres, boxes), mg.Field(dim, spheres[:BLOCK], boxes)
    memo, memo64 = {}, {}

    def motion(frm, to, fld=field, cache=memo):
        key = (tuple(frm), tuple(to))
        if key not in cache:
            cache[key] = check_motion(fld, bounds, fraction, frm, to)
        return cache[key]

    rng = mg.ChaCha12Rng(seed, pid)
    tree = np.zeros((max_nodes + 1, dim), dtype=np.float64)
    tree[0] = P["start"]
    rows = [[float(v) for v in P["start"]]]
    parents, cost = [-1], [0.0]
    n = 1
    h_iter, w_wire = mg.FNV_BASIS, 0
    iterations = accepted = 0
    goal_node = -1
    k = dict.fromkeys(COUNTERS, 0)
    for _ in range(max_iterations):
        if n >= max_nodes:
            break
        q_rand = list(goal_c) if mg.random_bool(rng, goal_bias) else [mg.random_range(rng, lo, hi) for lo, hi in bounds]
        nearest, min_dist = mg._nearest(tree, n, q_rand, dim)
        q_near = rows[nearest]
        q_new = mg.interpolate(q_near, q_rand, max_distance / min_dist) if min_dist > max_distance else list(q_rand)
        ok = motion(q_near, q_new)
        g = ((mg.FNV_BASIS ^ nearest) * FNV_P) & M64
        for v in q_new:
            g = ((g ^ mg.f64_bits(v)) * FNV_P) & M64
        g = ((g ^ int(ok)) * FNV_P) & M64
        h_iter = (h_iter * FNV_P + g) & M64
        iterations += 1
        if not ok:
            continue
        accepted += 1
        dn = row_dists(q_new, tree[:n])
        neighbours = [int(i) for i in np.nonzero(dn < search_radius)[0]]
        k["longest_list"] = max(k["longest_list"], len(neighbours))
        k["long_lists"] += len(neighbours) > BLOCK
        c0 = cost[nearest] + float(dn[nearest])
        best_parent, min_cost = nearest, c0
        below = []                                    # (cost-through, position in the list) of the valid neighbours below c0
        for pos, i in enumerate(neighbours):          # choose parent, ascending index, strict <
            c = cost[i] + float(dn[i])
            if c < c0 and motion(rows[i], q_new):
                below.append((c, pos))
            if c < min_cost:
                if motion(rows[i], q_new):
                    min_cost, best_parent = c, i
                else:
                    k["rejected"] += 1
                    k["late_only"] += motion(rows[i], q_new, field64, memo64)
            elif c == min_cost and i != best_parent and motion(rows[i], q_new):
                k["parent_ties"] += 1
        if below:
            low = min(c for c, _ in below)
            blocks = [pos // BLOCK for c, pos in below if c == low]
            k["shared_minima"] += len(blocks) > 1
            k["cross_block_minima"] += len(set(blocks)) > 1
        k["changed_parents"] += best_parent != nearest
        tree[n] = q_new
        rows.append(q_new)
        parents.append(best_parent)
        cost.append(min_cost)
        new_idx = n
        n += 1
        rew_cnt = rew_sum = 0
        for i in neighbours:                          # rewire
            if i == best_parent:
                continue
            c2 = min_cost + float(dn[i])
            k["rewire_ties"] += c2 == cost[i]
            if c2 < cost[i]:
                if motion(q_new, rows[i]):
                    parents[i] = new_idx
                    cost[i] = c2
                    rew_cnt += 1
                    rew_sum += i
                else:
                    k["rejected"] += 1
                    k["late_only"] += motion(q_new, rows[i], field64, memo64)
        k["rewires"] += rew_cnt
        w = mg.FNV_BASIS
        for v in (best_parent, mg.f64_bits(min_cost), rew_cnt, rew_sum):
            w = ((w ^ v) * FNV_P) & M64
        w_wire = (w_wire * FNV_P + w) & M64
        if mg.distance(q_new, goal_c) <= goal_r:
            if goal_node < 0:
                goal_node = new_idx
            if stop_at_goal:
                break
    return dict(n=n, iterations=iterations, accepted=accepted, checksum=(h_iter + w_wire) & M64, goal_node=goal_node,
                states=tree[:n].copy(), parents=parents, cost=cost, counters={key: int(v) for key, v in k.items()})


@functools.lru_cache(maxsize=None)
def slab_replay(dim):
    return replay(slab_scene(dim), SEED, PIDS[0])


@functools.lru_cache(maxsize=None)
def reach_replay(dim, variant):
    return replay(reach_scene(dim, variant), SEED, PIDS[0])
