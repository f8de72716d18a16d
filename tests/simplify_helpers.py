"""The shortcut of include/oxmpl_hip.h (oxhip_rrt_batch_simplify_paths) restated in Python, and the scenes its tests share.
Test-side only; independent of any kernel."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 42
BUDGET = 100000          # iterations a stop-at-goal oracle run may take (every recorded problem solves far earlier)
STAR_ITERATIONS = 3000   # RRT* runs past its first solution so that rewiring has shaped the path


def span_of(L, max_span):
    return L - 1 if max_span == 0 else min(max_span, L - 1)


def shortcut_dp(L, valid, dist, max_span=0):
    """Raw path p_0 .. p_{L-1}; valid(i, j) is asked for 2 <= j - i <= span only (adjacent edges are valid without a check);
    dist(i, j) is the space's distance.  Returns (indices, raw_cost, simplified_cost, checks)."""
    if L == 0:
        return [], 0.0, 0.0, 0
    S = span_of(L, max_span)
    cost, par, checks = [0.0] * L, [0] * L, 0
    for j in range(1, L):
        best, best_i = float("inf"), None
        for i in range(max(0, j - S), j):          # ascending, strict '<': ties keep the lowest i
            if j - i == 1:
                ok = True
            else:
                ok = bool(valid(i, j))
                checks += 1
            if ok:
                c = cost[i] + dist(i, j)
                if c < best:
                    best, best_i = c, i
        cost[j], par[j] = best, best_i
    idx = [L - 1]
    while idx[-1] != 0:
        idx.append(par[idx[-1]])
    idx.reverse()
    raw = 0.0
    for j in range(1, L):
        raw = raw + dist(j - 1, j)
    return idx, raw, cost[L - 1], checks


def expected_checks(L, max_span):
    S = span_of(L, max_span) if L else 0
    return sum(L - d for d in range(2, S + 1))


def rn_scenes():
    from oxmpl_amd import scenarios
    return dict(config1=scenarios.config1(), config2=scenarios.config2(), wall=scenarios.wall())


def oracle_rrt(sc, pid, star_radius=None, max_nodes=10000, stop_at_goal=True):
    from oracle import oracle_py as orc
    if star_radius is None:
        o = orc.OracleRRT(sc["dim"], sc["bounds"], sc["max_distance"], sc["goal_bias"], sc["lvs_fraction"], max_nodes,
                          stop_at_goal, SEED, pid)
    else:
        o = orc.OracleRRTStar(sc["dim"], sc["bounds"], sc["max_distance"], sc["goal_bias"], star_radius, sc["lvs_fraction"],
                              max_nodes, stop_at_goal, SEED, pid)
    if sc["spheres"] is not None:
        o.set_spheres(*sc["spheres"])
    if sc["boxes"] is not None:
        o.set_boxes(*sc["boxes"])
    o.setup(sc["start"], sc["goal_centre"], sc["goal_radius"])
    return o


def oracle_shortcut(o, path, max_span=0):
    """the DP over the oracle's own check_motion and distance"""
    from oracle import oracle_py as orc
    return shortcut_dp(len(path), lambda i, j: o.check_motion(path[i], path[j]), lambda i, j: orc.distance(path[i], path[j]),
                       max_span)
