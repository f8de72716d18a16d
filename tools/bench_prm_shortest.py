#!/usr/bin/env python3
"""Many queries on one PRM roadmap answered with shortest paths: one oxhip_prm_solve_batch (the
breadth-first batch of section 17, untouched) next to one oxhip_prm_solve_batch_shortest (distance weights), both followed by
oxhip_prm_batch_get_paths, in the same process, on
  * BASELINE.json configs[4]: R^6, 32 hyperspheres, connection radius 2, [milestones] milestones, [Q] seeded queries;
  * the SO(3) fixture (one 44.9 degree cone, radius 0.5) at 16,384 milestones, Q / 4 seeded queries.
Wall clock and HIP events, best of 3 after a warm-up, with the spread; the edge weights are computed once, in the warm-up, and
reported on their own.  Refuses to print unless both batches returned the same statuses and no shortest path costs more than the
breadth-first one.

Usage: bench_prm_shortest.py [Q=1024] [milestones=50000] [--out FILE=profiles/prm_shortest/bench_prm_shortest.json]"""
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from oxmpl_amd import capi, scenarios  # noqa: E402

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "prm_shortest", "bench_prm_shortest.json")
if OUT in argv:
    argv.remove(OUT)
Q = int(argv[0]) if len(argv) > 0 else 1024
N = int(argv[1]) if len(argv) > 1 else 50000
SEED, REP = 20261016, 3
PHASES = ("weights", "flags", "labels", "levels", "paths", "copies")


def run(g, starts, goals, radii, shortest):
    t0 = time.perf_counter()
    status = (g.solve_batch_shortest if shortest else g.solve_batch)(starts, goals, radii).copy()
    off, nodes, rows = g.batch_paths()
    wall = (time.perf_counter() - t0) * 1e3
    out = dict(wall=wall, status=status, off=off, nodes=nodes, rows=rows, timing=g.batch_last_timing())
    if shortest:
        out.update(cost=g.batch_costs().copy(), stats=g.batch_search_stats())
    return out


def path_costs(run_, dist):
    """the left-to-right cost of every path of a batch"""
    d = dist(run_["rows"][:-1], run_["rows"][1:]) if len(run_["rows"]) > 1 else np.zeros(0)
    out = np.full(len(run_["status"]), np.inf)
    for q in range(len(out)):
        a, b = int(run_["off"][q]), int(run_["off"][q + 1])
        if b > a:
            c = d[a]
            for v in d[a + 1:b - 1]:
                c = c + v
            out[q] = c
    return out


def measure(name, g, starts, goals, radii, dist):
    starts, goals, radii = (np.ascontiguousarray(a, dtype=np.float64) for a in (starts, goals, radii))
    n, entries, _ = g.sizes()
    run(g, starts, goals, radii, False)                         # warm-up of both; the shortest one computes the edge weights
    weights_ms = run(g, starts, goals, radii, True)["stats"]["phase_ms"][0]
    bfs = [run(g, starts, goals, radii, False) for _ in range(REP)]
    sp = [run(g, starts, goals, radii, True) for _ in range(REP)]
    for r in bfs[1:] + sp:
        if not np.array_equal(r["status"], bfs[0]["status"]):
            raise SystemExit("%s: the two batches disagree on a status -- nothing to report" % name)
    for r in sp[1:]:
        if not (np.array_equal(r["nodes"], sp[0]["nodes"]) and np.array_equal(r["cost"].view(np.uint64), sp[0]["cost"].view(np.uint64))):
            raise SystemExit("%s: two shortest-path batches differ -- nothing to report" % name)
    ok = bfs[0]["status"] == capi.OK
    c_bfs, c_sp = path_costs(bfs[0], dist), path_costs(sp[0], dist)
    if np.any(c_sp[ok] > c_bfs[ok] * (1.0 + 1e-12)) or not np.allclose(c_sp[ok], sp[0]["cost"][ok], rtol=1e-12):
        raise SystemExit("%s: a shortest path costs more than the breadth-first one -- nothing to report" % name)
    bw, sw = [r["wall"] for r in bfs], [r["wall"] for r in sp]
    best_b, best_s = bfs[int(np.argmin(bw))], sp[int(np.argmin(sw))]
    searched = bfs[0]["status"] != capi.ERR_INVALID_START_STATE
    rounds, relax = best_s["stats"]["label_rounds"][searched], best_s["stats"]["relaxations"][searched].astype(np.float64)
    ratio = c_bfs[ok] / c_sp[ok]
    phase = dict(zip(PHASES, best_s["stats"]["phase_ms"]))
    phase["weights"] = 0.0
    return {
        "roadmap": name, "milestones": n, "edge_entries": entries, "mean_degree": entries / n, "queries": len(radii),
        "solved": int(ok.sum()), "no_solution": int(np.sum(bfs[0]["status"] == capi.ERR_NO_SOLUTION_FOUND)),
        "invalid_start": int(np.sum(~searched)),
        "bfs_batch": {"wall_ms": bw, "wall_ms_best": min(bw), "wall_ms_spread": max(bw) - min(bw),
                      "phase_ms": dict(zip(("flags", "search", "paths", "copies"), best_b["timing"]["phase_ms"]))},
        "shortest_batch": {"wall_ms": sw, "wall_ms_best": min(sw), "wall_ms_spread": max(sw) - min(sw), "phase_ms": phase,
                           "edge_weights_once_ms": weights_ms, "edge_weights_bytes": 8 * entries, "rounds": best_s["timing"]["rounds"]},
        "shortest_over_bfs_wall": min(sw) / min(bw),
        "label_rounds_per_query": {"mean": float(rounds.mean()), "max": int(rounds.max())},
        "relaxations_per_edge_entry": {"mean": float(relax.mean() / entries), "max": float(relax.max() / entries)},
        "bfs_cost_over_shortest_cost": {"mean": float(ratio.mean()), "max": float(ratio.max()),
                                        "paths_that_differ": int(np.sum(ratio > 1.0))},
        "path_states_mean": {"bfs": float(np.diff(bfs[0]["off"].astype(np.int64))[ok].mean()),
                             "shortest": float(np.diff(sp[0]["off"].astype(np.int64))[ok].mean())},
    }


def rn_dist(a, b):
    acc = np.zeros(len(a))
    for k in range(a.shape[1]):
        d = a[:, k] - b[:, k]
        acc = acc + d * d
    return np.sqrt(acc)


def so3_dist(a, b):
    return capi.so3_op_batch(0, a, b) if len(a) else np.zeros(0)


def main():
    out = {"tool": "tools/bench_prm_shortest.py", "seed": SEED, "repetitions": REP, "rows": []}
    sc = scenarios.config5()
    g = scenarios.make_prm(sc, N)
    g.construct_roadmap()
    rng = np.random.default_rng(SEED)
    starts = rng.uniform(0.0, 10.0, size=(Q, 6))
    goals = rng.uniform(0.0, 10.0, size=(Q, 6))
    radii = rng.uniform(1.5, 2.5, size=Q)
    out["rows"].append(measure("config 5: R^6, 32 hyperspheres, radius 2", g, starts, goals, radii, rn_dist))
    g.close()
    q3 = max(1, Q // 4)
    g = capi.PRMRoadmap(4, [0.0, 0.0, 0.0, 1.0, math.pi], 0.5, 16384, lvs_fraction=0.05, seed=11, stream=0, space=capi.SPACE_SO3)
    g.set_spheres([[0.0, 0.0, 0.0, 1.0]], [44.9 * (math.pi / 180.0)])
    rng = np.random.default_rng(SEED)
    starts = rng.standard_normal(size=(q3, 4))
    goals = rng.standard_normal(size=(q3, 4))
    starts /= np.linalg.norm(starts, axis=1, keepdims=True)
    goals /= np.linalg.norm(goals, axis=1, keepdims=True)
    radii = rng.uniform(0.2, 0.6, size=q3)
    g.setup(starts[0], goals[0], float(radii[0]))
    g.construct_roadmap()
    out["rows"].append(measure("SO(3) fixture: one 44.9 degree cone, radius 0.5", g, starts, goals, radii, so3_dist))
    g.close()
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
