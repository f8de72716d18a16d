"""Planted paths for the extraction and the shortcutter (path_simplify.hip) at the limits that paths taken from a
solve never reach: DP windows wider than the wave, exact cost ties, every dimension, more than 64 spheres next to boxes, states far outside
the bounds, chords of length zero, slot counts on either side of a 64-bit word, rounds that mix problems with and without pairs.

Constructions only (numpy): nothing here loads the GPU library or the oracle.  What every scene is claimed to hold is computed with the CPU
oracle by tests/test_simplify_limits_model.py; tests/golden/make_golden_simplify_limits.py records the oracle's results and
tests/test_gpu_simplify_limits.py runs the scenes on the device.  A scene is a dict
    dim, so3, bounds, lvs_fraction, spheres (centres [n][dim], radii [n]) (SO(3): the cones), boxes (lo, hi) or None, max_nodes,
    problems [dict(path [L][dim] or None when unsolved, states, parents, goal (centre, radius), goal_node)],
    spans (the max_span values the tests run), matrix (True: the golden file records the whole verdict matrix)
Scenes are built once (functools caches) and shared: never modify one.

A path is planted as a tree (set_tree) whose parent chain from the goal node is the path: plant() below."""
import functools
import math

import numpy as np

import rrt_revalidate_helpers as rh

LANES = 64
GOAL_R = 2.0 ** -10          # R^n goal radius: the lattices below are 1/64 or coarser, so only the goal node itself satisfies it
SO3_GOAL_R = 1e-4
FULL = 2 ** 32 - 1


# ----------------------------------------------------------------------------------------------------------------- planting
def _so3_angle(a, b):
    return math.acos(min(1.0, abs(float(np.dot(a, b)))))


def plant(path, decoys, seed, so3=False, unsolved_goal=None):
    """-> (states [n][dim], parents [n], goal (centre, radius), goal_node).  The path's nodes sit at increasing tree indices with `decoys`
    further nodes scattered between them; a decoy hangs off any node of lower index, so the chain from the goal node is a gather.  The
    goal is a small ball about the last path state that no other node of index >= 1 satisfies; with `unsolved_goal` it is a ball about
    that centre, which no node satisfies (goal_node -1)."""
    path = np.ascontiguousarray(path, dtype=np.float64)
    L, dim = path.shape
    rng = np.random.RandomState(seed)
    n = L + decoys
    while True:   # (drawn again until some path node does not follow its predecessor directly)
        pos = np.concatenate([[0], np.sort(rng.choice(np.arange(1, n), L - 1, replace=False))]).astype(np.int64)
        if decoys == 0 or (np.diff(pos) > 1).any():
            break
    slot = {int(i): k for k, i in enumerate(pos)}
    states, parents = np.zeros((n, dim)), np.full(n, -1, dtype=np.int32)
    for i in range(n):
        if i in slot:
            k = slot[i]
            states[i] = path[k]
            parents[i] = pos[k - 1] if k else -1
        else:
            par = int(rng.randint(0, i))
            parents[i] = par
            if so3:
                q = rh.quat_mul(states[par], rh.quat_axis_half(rng.normal(size=3), 0.05))
                states[i] = q / math.sqrt(float(q @ q))
            else:
                step = rng.randint(1, 9, size=dim) * rng.choice([-1.0, 1.0], size=dim) / 16.0
                states[i] = states[par] + step
    radius = SO3_GOAL_R if so3 else GOAL_R
    centre = path[-1].copy() if unsolved_goal is None else np.asarray(unsolved_goal, dtype=np.float64)
    hit = [i for i in range(1, n)
           if (_so3_angle(states[i], centre) if so3 else math.sqrt(float(np.sum((states[i] - centre) ** 2)))) <= 16.0 * radius]
    goal_node = int(pos[-1]) if unsolved_goal is None else -1
    assert hit == ([goal_node] if goal_node >= 0 else []), (hit, goal_node)
    return states, parents, (centre, radius), goal_node


def _problem(path, decoys, seed, so3=False, unsolved_goal=None):
    states, parents, goal, goal_node = plant(path, decoys, seed, so3, unsolved_goal)
    return dict(path=None if unsolved_goal is not None else np.ascontiguousarray(path, dtype=np.float64), states=states, parents=parents,
                goal=goal, goal_node=goal_node)


def _scene(dim, bounds, lvs_fraction, spheres, boxes, problems, spans, matrix=False, so3=False, max_nodes=None):
    c = np.ascontiguousarray([s[0] for s in spheres], dtype=np.float64).reshape(len(spheres), dim)
    r = np.ascontiguousarray([s[1] for s in spheres], dtype=np.float64)
    bx = None
    if boxes:
        bx = (np.ascontiguousarray([b[0] for b in boxes], dtype=np.float64), np.ascontiguousarray([b[1] for b in boxes], dtype=np.float64))
    return dict(dim=dim, so3=so3, bounds=bounds, lvs_fraction=lvs_fraction, spheres=(c, r), boxes=bx, problems=problems, spans=tuple(spans),
                matrix=matrix, max_nodes=max_nodes or max(len(p["parents"]) for p in problems) + 8)


def length(problem):
    return 0 if problem["path"] is None else len(problem["path"])


def wide_span(L):
    """a window wider than the wave, where the path allows one below its full span"""
    return LANES + 1 if L > LANES + 2 else None


def spans_for(L):
    return tuple(s for s in (0, wide_span(L), 2) if s is not None)


R2 = [(0.0, 64.0)] * 2


# ----------------------------------------------------------------------------------------------------------------- R^2 paths
def corner_path():
    """100 nodes along y = 8 from x = 1 in steps of 1/4, then 100 nodes up x = 25.75: every cost is a sum of quarters, exactly"""
    k = np.arange(100)
    a = np.stack([1.0 + 0.25 * k, np.full(100, 8.0)], axis=1)
    b = np.stack([np.full(100, 25.75), 8.25 + 0.25 * k], axis=1)
    return np.concatenate([a, b])


def line_path(L):
    return np.stack([1.0 + 0.25 * np.arange(L), np.full(L, 8.0)], axis=1)


def arc_path(L, a0=0.1, a1=3.0):
    """points of the circle of radius 20 about (32, 32), rounded to 1/64"""
    t = np.linspace(a0, a1, L)
    return np.round(np.stack([32.0 + 20.0 * np.cos(t), 32.0 + 20.0 * np.sin(t)], axis=1) * 64.0) / 64.0


ARC_DISC = [([32.0, 32.0], 17.0)]
CORNER_SPANS = (1, 2, 63, 64, 65, 70, 198, 199, 200, FULL)       # L = 200: L - 2, L - 1, L among them; 0 is run as well
ARC_SPANS_L = 200                                                  # the arc problem that runs the same list


@functools.lru_cache(maxsize=None)
def corner_r2():
    """The tie scene.  One box fills the inside of the corner, so a chord between the legs is valid only close to the corner, and along
    a leg every split of a stretch costs the same, bit for bit.  At full span: idx [0, 98, 100, 199]; 196 of the 199 steps tie among
    valid candidates, in 98 the winner is not the window's first index, in 70 two tying candidates sit 64 apart (one lane holds both),
    in 70 the parent lies more than 64 below its child; 9802 pairs are valid and 9899 invalid.  max_span 70: [0, 28, 98, 100, 129, 199]."""
    box = ([0.0, 8.125], [25.625, 40.0])
    return _scene(2, R2, 0.05, [], [box], [_problem(corner_path(), 60, 11)], (0,) + CORNER_SPANS, matrix=True)


LINE_LENGTHS = (66, 130, 200)


@functools.lru_cache(maxsize=None)
def line_free_r2():
    """Straight lines of quarters with one sphere far away (the checker runs, and passes everything): every pair is valid and every
    step ties over its whole window, so idx is [0, L - 1] at full span and par[j] = max(0, j - S) under a window S."""
    probs = [_problem(line_path(L), L // 4, 20 + L) for L in LINE_LENGTHS]
    return _scene(2, R2, 0.05, [([60.0, 60.0], 1.0)], [], probs, (0, 65, 2))


ARC_LENGTHS = (66, 130, 200, 257)


@functools.lru_cache(maxsize=None)
def arc_r2():
    """Arcs about a disc: chords are valid up to an index distance that grows with L, both verdicts in thousands, and from L = 200 on
    dozens of parents lie more than 64 below their child."""
    probs = [_problem(arc_path(L), L // 4, 40 + L) for L in ARC_LENGTHS]
    return _scene(2, R2, 0.05, ARC_DISC, [], probs, (0, 65, 2) + CORNER_SPANS)


WORD_LENGTHS = (2, 3, 4, 63, 64, 65, 66, 67, 127, 128, 129)
WORD_SPANS = (0, 2, 3)


def slot_count(L, max_span):
    """slots of a problem's pair matrix: (S - 1) * L, none below S = 2"""
    if L < 3:
        return 0
    S = L - 1 if max_span == 0 else min(max_span, L - 1)
    return (S - 1) * L if S >= 2 else 0


def word_residues():
    """(L, span) -> slots mod 64 for the paths of word_edges"""
    return {(L, s): slot_count(L, s) % LANES for L in WORD_LENGTHS for s in WORD_SPANS}


# which (L, span) end exactly on a word, one slot short of one and one slot past one
WORD_ON = [(64, 0), (64, 2), (64, 3), (66, 0), (128, 0), (128, 2), (128, 3)]
WORD_SHORT = [(63, 2), (65, 0), (127, 2), (129, 0)]
WORD_PAST = [(65, 2), (129, 2)]


@functools.lru_cache(maxsize=None)
def word_edges():
    """Short arcs about the disc, one problem per length: with spans 0, 2 and 3 their slot counts end on a word, one short and one past"""
    probs = [_problem(arc_path(L), 6, 60 + L) for L in WORD_LENGTHS]
    return _scene(2, R2, 0.05, ARC_DISC, [], probs, WORD_SPANS)


@functools.lru_cache(maxsize=None)
def full_tree_r2():
    """max_nodes = 1024 and a chain of exactly 1024 nodes, every one on the path: chain_length's cnt >= n guard at its edge.  The disc
    nearly fills the circle, so within a span of 96 the longer chords already fail."""
    return _scene(2, R2, 0.05, [([32.0, 32.0], 19.875)], [], [_problem(arc_path(1024), 0, 70)], (96,), max_nodes=1024)


MIXED_LENGTHS = (0, 2, 3, 130, 0, 2, 66)
MIXED_CHUNKS = (0, 1, 2, 3, 7)


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """Seven problems among the arc's disc; lengths 0 (unsolved), 2, 3, 130, 0, 2, 66.  Problems without pairs (L < 3) open a round
    (chunks 2, 3, 7, 0), sit between the two long ones (chunks 7, 0) and close a round (chunks 2 and 3), and with chunk 1 they are
    rounds of their own."""
    probs = []
    for p, L in enumerate(MIXED_LENGTHS):
        if L == 0:
            probs.append(_problem(arc_path(5 + p), 4, 80 + p, unsolved_goal=[60.0, 4.0]))
        else:
            probs.append(_problem(arc_path(L, 0.1 + 0.01 * p), max(2, L // 4), 80 + p))
    return _scene(2, R2, 0.05, ARC_DISC, [], probs, (0, 2))


def round_word_offsets(lengths, max_span, chunk):
    """woff of every round of simplify_paths(max_span, chunk): a prefix sum of the problems' words"""
    words = [-(-slot_count(L, max_span) // LANES) for L in lengths]
    step = chunk or len(lengths)
    return [[sum(words[q:q + k]) for k in range(len(words[q:q + step]) + 1)] for q in range(0, len(lengths), step)]


# ----------------------------------------------------------------------------------------------------------------- every dimension
DIMS = tuple(range(2, 9))
DIMS_L = 70
DIMS_FAR = (65, 66, 67, 68)       # path indices of the four far nodes
DIMS_TWINS = (30, 32)             # equal coordinates: a chord of length 0
DIMS_WIDTH = 64.0
DIMS_LAST_AXIS = 66               # the far node that is large in the last axis only
DIMS_BOX_C = 2                    # the box that alone decides chords near the arc's end
DIMS_WALL_R = 2000.0


@functools.lru_cache(maxsize=None)
def dims(D):
    """L = 70 at full span in R^D: 65 nodes on an arc in the (x0, x1) plane with small lattice offsets in the other axes, four nodes
    1000 to 10000 bound-widths outside the bounds (node 66 in the last axis only), and the last node back on the arc.  72 spheres: the
    central ball; two very large ones just outside the bounds, which cut every chord from the arc to a far node within its first steps;
    one about each of the far nodes 65 and 67, which cuts every chord that leaves it (so only 66 -> 68, valid, and 66 -> 69 run their
    thousands of steps); 59 that no chord reaches; and eight of index 64 .. 71 on a ring inside the arc, in the second 64-block of the
    midpoint filter.  3 boxes inside the bounds.  Nodes 30 and 32 are equal."""
    W, R = DIMS_WIDTH, DIMS_WALL_R
    t = np.concatenate([np.linspace(0.1, 2.8, 65), [3.0] * 5])
    path = np.full((DIMS_L, D), 32.0)
    path[:, 0] = np.round((32.0 + 20.0 * np.cos(t)) * 64.0) / 64.0
    path[:, 1] = np.round((32.0 + 20.0 * np.sin(t)) * 64.0) / 64.0
    k = np.arange(DIMS_L)
    for d in range(2, D):
        path[:, d] = 32.0 + ((k * (d + 3)) % 7 - 3) / 4.0
    path[DIMS_TWINS[1]] = path[DIMS_TWINS[0]]
    base = np.full(D, 32.0)
    far = [base.copy() for _ in range(4)]
    far[0][0] = -1e4 * W
    far[1][D - 1] = W + 1e3 * W
    far[2][0], far[2][1] = -3e3 * W, 40.0
    far[3][0], far[3][1] = -1e3 * W, 24.0
    for i, f in zip(DIMS_FAR, far):
        path[i] = f
    assert DIMS_FAR[1] == DIMS_LAST_AXIS
    plane = lambda radius, angle: [32.0 + radius * math.cos(angle), 32.0 + radius * math.sin(angle)] + [32.0] * (D - 2)  # noqa: E731
    wall_a, wall_b = base.copy(), base.copy()
    wall_a[0] = -50.0 - R
    wall_b[D - 1] = W + 50.0 + R
    spheres = [(base, 11.0), (wall_a, R), (wall_b, R), (far[0], 200.0), (far[2], 200.0)]
    spheres += [(plane(27.0, 0.1 * j), 0.5) for j in range(5, 64)] + [(plane(15.0, 0.3 + 0.25 * m), 2.5) for m in range(8)]

    def box(radius, angle, half):
        cx, cy = plane(radius, angle)[:2]
        return ([cx - half, cy - half] + [0.0] * (D - 2), [cx + half, cy + half] + [64.0] * (D - 2))

    boxes = [box(12.5, 1.0, 1.5), box(15.0, 2.3, 1.0), box(17.5, 2.5, 2.0)]
    return _scene(D, [(0.0, W)] * D, 0.5, spheres, boxes, [_problem(path, 20, 100 + D)], (0, 65, 2), matrix=True)


BAD_EDGE = (5, 6)


@functools.lru_cache(maxsize=None)
def bad_adjacent_r3():
    """A zigzag in R^3 and, set after planting, a wall across the whole space between nodes 5 and 6: check_motion fails that edge and
    every chord over it, the shortcutter takes the edge as the planner's ("true without a check"), so the result holds 5 and 6."""
    k = np.arange(12)
    path = np.stack([1.0 + 0.5 * k, 5.0 + 1.5 * (k % 2), 5.0 + 0.25 * (k % 3)], axis=1)
    mid = 0.5 * (path[BAD_EDGE[0]][0] + path[BAD_EDGE[1]][0])
    wall = ([mid - 0.125, -1.0, -1.0], [mid + 0.125, 11.0, 11.0])
    return _scene(3, [(0.0, 10.0)] * 3, 0.05, [([2.25, 4.625, 5.0], 0.4375)], [wall], [_problem(path, 6, 120)], (0, 2, 3), matrix=True)


# ----------------------------------------------------------------------------------------------------------------- SO(3)
SO3_L = 70
SO3_TWINS = (38, 40)      # equal as rotations, opposite in sign
SO3_SWITCH_PAIR = (10, 12)
SO3_SWITCH_OFF = 5e-7     # the pair's distance is acos(0.9995) + this: its dot product lies within 1e-6 below 0.9995


@functools.lru_cache(maxsize=None)
def so3_arc():
    """Rotations about a fixed axis, half-angles 0.05 .. 1.2, each nudged off the axis by a small rotation of its own; every odd node is
    stored as -q.  Node 40 is -(node 38): distance 0.  Node 12 is node 10 turned by acos(0.9995) + 5e-7, where interpolate changes its
    branch.  Three cones sit on the arc between nodes, so chords across them fail and chords between them pass."""
    rng = np.random.RandomState(7)
    axis = np.array([1.0, 2.0, 3.0])
    h = 0.05 + (1.15 / (SO3_L - 1)) * np.arange(SO3_L)
    q = np.zeros((SO3_L, 4))
    for k in range(SO3_L):
        v = rh.quat_mul(rh.quat_axis_half(axis, h[k]), rh.quat_axis_half(rng.normal(size=3), 0.003))
        q[k] = v / math.sqrt(float(v @ v))
    a, b = SO3_SWITCH_PAIR
    v = rh.quat_mul(q[a], rh.quat_axis_half(axis, rh.SO3_SWITCH + SO3_SWITCH_OFF))
    q[b] = v / math.sqrt(float(v @ v))
    q[1::2] *= -1.0
    q[SO3_TWINS[1]] = -q[SO3_TWINS[0]]
    cones = [(rh.quat_axis_half(axis, 0.5 * (h[m] + h[m + 1])), 0.012) for m in (20, 45)] + [(rh.quat_axis_half(axis, h[60] + 0.004), 0.02)]
    return _scene(4, None, 0.1, cones, [], [_problem(q, 16, 130, so3=True)], (0, 65, 2), matrix=True, so3=True)


def scenes():
    """name -> thunk"""
    out = dict(corner_r2=corner_r2, line_free_r2=line_free_r2, arc_r2=arc_r2, word_edges=word_edges, full_tree_r2=full_tree_r2,
               mixed_batch=mixed_batch, bad_adjacent_r3=bad_adjacent_r3, so3_arc=so3_arc)
    for D in DIMS:
        out["dims_r%d" % D] = functools.partial(dims, D)
    return out


def spans_of(name, scene, p):
    """the spans the golden file records for problem p: the scene's list, the long span lists on corner_r2 and one arc only"""
    L = length(scene["problems"][p])
    if name == "arc_r2" and L != ARC_SPANS_L:
        return (0, 65, 2)
    if name == "line_free_r2":
        return spans_for(L)
    return tuple(dict.fromkeys(scene["spans"]))
