"""The numpy half of the oracle for oxhip_rrt_batch_revalidate_trees, and the planted trees the tests
share.  Nothing here calls the code under test: the edge verdicts come from a check_motion the caller brings (the batch's own
entry point on the GPU, the pure-Python restatements in tests/golden/make_golden_rrt_revalidate.py), the goal test likewise;
survival, compaction, remapping, skip flags and the goal node are plain loops over them.

The planted scenes put three trees into ONE obstacle field (a batch has one): tree A lives where no obstacle is, tree B has every
node but its root inside one large obstacle, tree C is the shape under test with small obstacles on chosen nodes."""
import math

import numpy as np


# ------------------------------------------------------------------------------------------------ the plain semantics
def prune(states, parents, edge_ok):
    """edge_ok[i] (i >= 1): verdict of check_motion(parent[i] -> i).  Node 0 stays; node i stays iff edge_ok[i] and its parent
    stays.  -> dict(alive, new_index, states, parents) with survivors in their old order and parents remapped."""
    states = np.asarray(states, dtype=np.float64)
    parents = np.asarray(parents, dtype=np.int32)
    n = len(parents)
    alive = np.zeros(n, dtype=bool)
    alive[0] = True
    for i in range(1, n):   # parents precede children
        alive[i] = bool(edge_ok[i]) and alive[parents[i]]
    new_index = np.full(n, -1, dtype=np.int32)
    new_index[alive] = np.arange(int(alive.sum()), dtype=np.int32)
    kept_parents = np.array([-1 if parents[i] < 0 else new_index[parents[i]] for i in range(n) if alive[i]], dtype=np.int32)
    return dict(alive=alive, new_index=new_index, states=np.ascontiguousarray(states[alive]), parents=kept_parents)


def skip_flags(states):
    """what set_tree computes: a node carries the flag iff a node of lower index has equal coordinates (as values: -0.0 == 0.0)"""
    states = np.asarray(states, dtype=np.float64)
    seen, out = {}, np.zeros(len(states), dtype=np.uint8)
    for i, row in enumerate(states):
        key = tuple(float(v) + 0.0 for v in row)
        out[i] = 1 if key in seen else 0
        seen.setdefault(key, i)
    return out


def goal_node(satisfied):
    """lowest index i >= 1 whose state satisfies the goal, -1 if none (the root is not counted)"""
    for i in range(1, len(satisfied)):
        if satisfied[i]:
            return i
    return -1


def expected(states, parents, edge_ok, satisfied):
    """everything the call leaves for one problem; `satisfied[i]`: goal.is_satisfied(old node i)"""
    edge_ok = np.asarray(edge_ok, dtype=bool).copy()
    edge_ok[0] = True
    pr = prune(states, parents, edge_ok)
    sat_after = np.asarray(satisfied, dtype=bool)[pr["alive"]]
    return dict(edge_ok=edge_ok, new_index=pr["new_index"], states=pr["states"], parents=pr["parents"], skip=skip_flags(pr["states"]),
                goal_node=goal_node(sat_after), n_removed=int(len(parents) - pr["alive"].sum()), n=int(pr["alive"].sum()))


def edge_rows(states, parents):
    """(from rows, to rows) of the edges 1 .. n - 1, the direction the planner checked them in"""
    states = np.asarray(states, dtype=np.float64)
    parents = np.asarray(parents, dtype=np.int32)
    return states[parents[1:]], states[1:]


# ------------------------------------------------------------------------------------------------ planted trees
BOUNDS_LO, BOUNDS_HI = 0.0, 10.0
KILL_R = 0.02          # radius of the small obstacle that sits on a node (its edge's `to` state is always tested)
BIG_R = 1.4            # the obstacle that holds tree B


def _rng(seed):
    return np.random.RandomState(seed)


def topology(kind, n, rng):
    """parents[n] of the named shape (parents precede children)"""
    par = np.full(n, -1, dtype=np.int32)
    for i in range(1, n):
        if kind == "chain":
            par[i] = i - 1
        elif kind == "star":
            par[i] = 0
        elif kind == "interleave":      # two subtrees under the root whose nodes alternate in index order: odd under 1, even under 2
            par[i] = 0 if i <= 2 else i - 2
        else:                           # "random"
            par[i] = rng.randint(0, i)
    return par


def rn_tree(dim, n, kind, region, seed):
    """n states of R^dim with coordinate 0 inside `region` = (lo, hi) and the others in [1, 9] (tree B: all near the big obstacle's
    centre), and the shape's parents"""
    rng = _rng(seed)
    s = rng.uniform(1.0, 9.0, size=(n, dim))
    s[:, 0] = rng.uniform(region[0], region[1], size=n)
    if kind == "chain" and dim >= 2:
        # a snake of short edges (rows of 64 nodes, 0.2 apart), so that an obstacle on one node fails that node's edge alone
        i = np.arange(n)
        col = np.where((i // 64) % 2 == 0, i % 64, 63 - i % 64)
        s[:, 0] = region[0] + (region[1] - region[0]) * col / 64.0
        s[:, 1] = 1.0 + 0.2 * (i // 64)
        s[:, 2:] = 5.0
    return np.ascontiguousarray(s), topology(kind, n, rng)


def rn_scene(dim, n, kind, kill, seed, boxes=False, goal="none", twins=()):
    """three trees and an obstacle field for R^dim: -> dict(trees=[(states, parents)] * 3, spheres, boxes, goals=[(centre, radius)] * 3)
    kill: indices of tree C whose own state gets a small obstacle (sphere, or box when `boxes`).
    twins: (low, high) index pairs of tree C made equal in coordinates.
    goal: "none" | "kept" (around a node that survives above removed ones) | "lost" (around a killed node) | "root" (around the
    root only)."""
    a_states, a_par = rn_tree(dim, n, kind, (0.5, 3.0), seed)
    c_states, c_par = rn_tree(dim, n, kind, (3.6, 6.4), seed + 1)
    b_states, b_par = rn_tree(dim, n, kind, (8.0, 9.0), seed + 2)
    b_states[:, 1:] = 4.8 + 0.4 * (b_states[:, 1:] - 1.0) / 8.0
    b_states[0, 0] = 6.7   # (the root is never tested: it may sit anywhere)
    for lo, hi in twins:
        c_states[hi] = c_states[lo]
    big_c = np.array([8.5] + [5.0] * (dim - 1))
    spheres = [(big_c, BIG_R)]
    box_list = []
    for k in kill:
        if boxes:
            box_list.append((c_states[k] - KILL_R, c_states[k] + KILL_R))
        else:
            spheres.append((c_states[k].copy(), KILL_R))
    goals = [(np.full(dim, 5.0), 0.0)] * 3
    far = np.array([9.9] + [0.1] * (dim - 1))
    g = (far, 0.01)
    if goal == "kept":
        g = (c_states[n - 1].copy(), 0.01)
    elif goal == "lost":
        g = (c_states[kill[0]].copy(), 0.01)
    elif goal == "root":
        g = (c_states[0].copy(), 0.01)
    goals = [(far, 0.01), (far, 0.01), g]
    return dict(dim=dim, trees=[(a_states, a_par), (b_states, b_par), (c_states, c_par)], spheres=spheres, boxes=box_list, goals=goals)


# ---- SO(3): unit quaternions (x, y, z, w)
def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def quat_axis_half(axis, half):
    """rotation about `axis` whose SO(3) distance from the identity is `half` (half the rotation angle)"""
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / math.sqrt(float(axis @ axis))
    q = np.concatenate([axis * math.sin(half), [math.cos(half)]])
    return q / math.sqrt(float(q @ q))


SO3_CENTRES = [np.array([0.0, 0.0, 0.0, 1.0]), np.array([0.0, 0.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0, 0.0])]   # trees A, B, C
SO3_BIG_R = 0.5
SO3_KILL_R = 0.004
SO3_SWITCH = math.acos(0.9995)   # so3 interpolate takes its near-parallel branch above this dot product


def so3_tree(n, kind, centre, spread, seed, switch_pairs=False):
    """n rotations within `spread` (SO(3) distance) of `centre`.  switch_pairs: every node from 3 on is its parent turned by a
    half-angle within 1e-6 .. 1e-4 of acos(0.9995), on either side: pairs where interpolate changes its branch."""
    rng = _rng(seed)
    par = topology(kind, n, rng)
    s = np.zeros((n, 4))
    for i in range(n):
        if switch_pairs and i >= 3:
            half = SO3_SWITCH + (1e-6, -1e-6, 1e-4, -1e-4, 0.0)[i % 5]
            q = quat_mul(s[par[i]], quat_axis_half(rng.normal(size=3), half))
        else:
            q = quat_mul(centre, quat_axis_half(rng.normal(size=3), rng.uniform(0.02, spread)))
        s[i] = q / math.sqrt(float(q @ q))
    return s, par


def so3_scene(n, kind, kill, seed, goal="none", switch_pairs=False, twins=()):
    a = so3_tree(n, kind, SO3_CENTRES[0], 0.35, seed)
    b = so3_tree(n, kind, SO3_CENTRES[1], 0.2, seed + 2)
    c = so3_tree(n, kind, SO3_CENTRES[2], 0.35, seed + 1, switch_pairs)
    for lo, hi in twins:
        c[0][hi] = c[0][lo]
    cones = [(SO3_CENTRES[1].copy(), SO3_BIG_R)] + [(c[0][k].copy(), SO3_KILL_R) for k in kill]
    far = quat_axis_half([0.0, 1.0, 0.0], 1.5)
    g = (far, 0.001)
    if goal == "kept":
        g = (c[0][n - 1].copy(), 0.001)
    elif goal == "lost":
        g = (c[0][kill[0]].copy(), 0.001)
    return dict(dim=4, trees=[a, b, c], spheres=cones, boxes=[], goals=[(far, 0.001), (far, 0.001), g])


# name -> a thunk that builds the scene.  "partial": tree C must lose some but not all of its nodes (recorded in the golden file)
def planted_scenes():
    out = {}
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025):
        kill = [k for k in ((1,) if n < 63 else (n // 3, n - 2)) if 1 <= k < n]
        out["r3_random_n%d" % n] = (lambda n=n, kill=kill: rn_scene(3, n, "random", sorted(set(kill)), 100 + n), n >= 63)
    for pos in (1, 1000, 2048):
        out["r2_chain2049_cut%d" % pos] = (lambda pos=pos: rn_scene(2, 2049, "chain", [pos], 300 + pos), pos != 1)
    out["r2_star"] = (lambda: rn_scene(2, 300, "star", [5, 100, 299], 400), True)
    out["r3_interleave"] = (lambda: rn_scene(3, 401, "interleave", [1], 410, goal="kept"), True)
    # the odd nodes die with node 1: (11, 40) and (11, 21) lose the lower twin, (10, 41) the higher one, (12, 50) neither, (13, 51) both
    out["r3_twins"] = (lambda: rn_scene(3, 80, "interleave", [1], 420, twins=[(11, 40), (11, 21), (10, 41), (12, 50), (13, 51)]), True)
    out["r3_goal_lost"] = (lambda: rn_scene(3, 90, "random", [45, 12], 440, goal="lost"), True)
    out["r3_goal_kept"] = (lambda: rn_scene(3, 90, "random", [7, 30], 450, goal="kept"), True)
    out["r3_goal_root"] = (lambda: rn_scene(3, 90, "random", [7, 30], 460, goal="root"), True)
    for dim in range(1, 9):
        out["r%d_spheres" % dim] = (lambda dim=dim: rn_scene(dim, 130, "random", [9, 77], 500 + dim, goal="kept"), True)
        out["r%d_boxes" % dim] = (lambda dim=dim: rn_scene(dim, 130, "random", [11, 64], 520 + dim, boxes=True), True)
    out["so3_random"] = (lambda: so3_scene(200, "random", [6, 90], 600, goal="kept"), True)
    out["so3_switch"] = (lambda: so3_scene(120, "chain", [70], 610, switch_pairs=True), True)
    out["so3_twins"] = (lambda: so3_scene(70, "interleave", [1], 620, goal="lost", twins=[(11, 40), (10, 41), (12, 50)]), True)
    return out
