"""The dense shortcut of include/oxmpl_hip.h (oxhip_prm_batch_simplify_paths) restated in Python, and the limit shapes its tests
share.  Test-side only; independent of any kernel.

A shape is a planted path in R^2: its points p_0 .. p_{L-1}, the spheres of its scene, and (m, max_span).  On the device it is a
chain roadmap of the milestones p_1 .. p_{L-1} and one query from p_0 (chain_roadmap / chain_query below)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BOUNDS = [(-2.0, 12.0), (-2.0, 12.0)]
FRACTION = 0.05
RADIUS = 1.5          # the start p_0 connects to p_1 alone: |p_0 p_1| < 1.5 <= |p_0 p_2| in every shape


def _dist2(a, b):
    return sum((x - y) * (x - y) for x, y in zip(a, b))


def span_of(L, max_span):
    return L - 1 if max_span == 0 else min(max_span, L - 1)


def dense_points(points, m, interp):
    """q_{k m} = p_k itself; q_{k m + r} = interp(p_k, p_{k+1}, r / m) with one divide"""
    pts = [np.array(p, dtype=np.float64) for p in points]
    if not pts:
        return []
    out = []
    for k in range(len(pts) - 1):
        out.append(pts[k])
        for r in range(1, m):
            out.append(np.array(interp(pts[k], pts[k + 1], float(r) / float(m)), dtype=np.float64))
    out.append(pts[-1])
    return out


def same_edge(u, v, m):
    return u // m == (v - 1) // m


def dense_shortcut(points, m, max_span, valid, dist, interp):
    """valid(a, b) is asked, in path order, for the pairs of the window that are not on one original edge; dist(a, b) is the
    space's distance; interp(a, b, t) its interpolation.  Returns dict(dense, idx, raw, simp, checks)."""
    L = len(points)
    if L == 0:
        return dict(dense=[], idx=[], raw=0.0, simp=0.0, checks=0)
    q = dense_points(points, m, interp)
    M = len(q)
    W = span_of(L, max_span) * m
    cost, par, checks = [0.0] * M, [0] * M, 0
    for v in range(1, M):
        best, best_u = float("inf"), None
        for u in range(max(0, v - W), v):              # ascending, strict '<': ties keep the lowest u
            if same_edge(u, v, m):
                ok = True
            else:
                ok = bool(valid(q[u], q[v]))
                checks += 1
            if ok:
                c = cost[u] + dist(q[u], q[v])
                if c < best:
                    best, best_u = c, u
        cost[v], par[v] = best, best_u
    idx = [M - 1]
    while idx[-1] != 0:
        idx.append(par[idx[-1]])
    idx.reverse()
    raw = 0.0
    for k in range(L - 1):
        raw = raw + dist(q[k * m], q[(k + 1) * m])
    return dict(dense=q, idx=idx, raw=raw, simp=cost[M - 1], checks=checks)


def expected_checks(L, m, max_span):
    """pairs with 1 <= d <= W, less the m (m + 1) / 2 per original edge that lie on one edge"""
    if L == 0:
        return 0
    M, W = (L - 1) * m + 1, span_of(L, max_span) * m
    return W * M - W * (W + 1) // 2 - (L - 1) * (m * (m + 1) // 2)


def matrix_bits(L, m, max_span):
    """(W - 1) * M: the slots of the bit matrix before padding to whole words"""
    M, W = (L - 1) * m + 1, span_of(L, max_span) * m
    return max(W - 1, 0) * M


# ---- the limit shapes

def zigzag(L):
    """p_k = (k, k odd).  Per corner p_{k+1} two spheres: one of radius 0.2 on the chord p_k -> p_{k+2} (the skip-one chords fail,
    longer ones pass) and one of radius 0.15 just inside the corner (the shortest links between the two edges fail, as a
    subdivided path with max_span = 1 needs)"""
    pts = [[float(k), float(k % 2)] for k in range(L)]
    centres, radii = [], []
    for k in range(L - 2):
        y = float(k % 2)                      # the chord's height; the corner is at 1 - y
        centres += [[float(k + 1), y], [float(k + 1), 0.7 - 0.4 * y]]
        radii += [0.2, 0.15]
    return pts, centres, radii


def corner_shape():
    """an L-shaped path round a sphere that blocks every chord from the first leg's first half to the second leg's second half:
    only a link between points inside the legs cuts the corner"""
    pts = [[0.0, 0.0], [1.25, 0.0], [2.5, 0.0], [2.5, 1.25], [2.5, 2.5]]
    return pts, [[1.25, 1.25]], [1.0]


def tie_shape():
    """mirror-symmetric about x = 1.5: the chains [0, 1, 3] and [0, 2, 3] cost fl(sqrt 2 + sqrt 5) and fl(sqrt 5 + sqrt 2), the same
    bits; the sphere under the path blocks p_0 -> p_3"""
    pts = [[0.0, 0.0], [1.0, 1.0], [2.0, 1.0], [3.0, 0.0]]
    return pts, [[1.5, -0.3]], [0.5]


# name -> (points, sphere centres, radii, m, max_span, what it exercises)
def limit_shapes():
    shapes = {}
    for bits_, (L, m, span) in {63: (9, 1, 0), 64: (4, 5, 1), 65: (5, 3, 2), 128: (6, 3, 3)}.items():
        pts, c, r = zigzag(L)
        shapes["matrix_%d" % bits_] = (pts, c, r, m, span, "(W - 1) M = %d slots: a word boundary of the bit matrix" % bits_)
    pts, c, r = corner_shape()
    shapes["corner_m1"] = (pts, c, r, 1, 0, "a corner that no link between waypoints cuts")
    shapes["corner_m8"] = (pts, c, r, 8, 0, "the same corner cut between waypoints")
    pts, c, r = tie_shape()
    shapes["tie"] = (pts, c, r, 1, 0, "two chains of equal cost bits: the lowest u wins")
    shapes["short_L2_m1"] = ([[0.0, 0.0], [1.0, 1.0]], [], [], 1, 0, "L = 2, m = 1: no pairs at all")
    shapes["short_L2_m2"] = ([[0.0, 0.0], [1.0, 1.0]], [], [], 2, 0, "L = 2, m = 2: every pair on one edge, no checks")
    shapes["short_L3_m1"] = ([[0.0, 0.0], [1.0, 1.0], [2.0, 0.0]], [[1.0, 0.0]], [0.2], 1, 0, "L = 3, m = 1: one pair")
    return shapes


def oracle_checker(centres, radii):
    """the CPU side's check_motion over a shape's scene (an OracleRRT of the same bounds and fraction; never solved)"""
    from oracle import oracle_py as orc
    o = orc.OracleRRT(2, BOUNDS, 0.5, 0.0, FRACTION, 16, True, 1, 0)
    if len(radii):
        o.set_spheres(np.array(centres, dtype=np.float64), np.array(radii, dtype=np.float64))
    o.setup([-1.0, -1.0], [11.0, 11.0], 0.1)
    return o


def model_of_shape(shape, checker=None):
    from oracle import oracle_py as orc
    pts, c, r, m, span, _ = shape
    o = checker or oracle_checker(c, r)
    return dense_shortcut(pts, m, span, lambda a, b: o.check_motion(a, b), orc.distance, orc.interpolate)


def chain_roadmap(points):
    """milestones p_1 .. p_{L-1} joined in a chain -> (states, offsets, neighbours) for set_roadmap"""
    ms = np.array(points[1:], dtype=np.float64)
    n = len(ms)
    nbrs, off = [], [0]
    for i in range(n):
        nbrs += [j for j in (i - 1, i + 1) if 0 <= j < n]
        off.append(len(nbrs))
    return ms, np.array(off, dtype=np.uint64), np.array(nbrs, dtype=np.uint32)


def chain_query(points):
    """(start, goal centre, goal radius): from p_0 to the last milestone alone"""
    return list(points[0]), list(points[-1]), 1e-6
