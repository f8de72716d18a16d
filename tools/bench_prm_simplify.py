#!/usr/bin/env python3
"""The answered paths of a PRM batch, subdivided and shortcut on the device, on BASELINE.json's config 5
(R^6, 32 spheres): a roadmap of [milestones] milestones, [Q] queries with random valid-or-not starts and goals, answered
breadth-first and with shortest paths, then oxhip_prm_batch_simplify_paths with subdivide in {1, 4, 16} and no max_span.
Per (batch kind, subdivide): the four phase times by HIP events (upload + subdivide, pair matrix, DP, copies) and the wall
clock of the call; beside them the solve-batch time of the same run, the yardstick for "post-processing costs no more than
planning"; the mean and worst simplified_cost / raw_cost.  One warm-up, then the median of five.
The host route -- batch_paths, one oxhip_prm_check_motion call over all pairs of the dense paths, the DP in Python -- is timed
on the first 32 answered queries and extrapolated to the batch by the number of checks: stated as extrapolated.

Usage: bench_prm_simplify.py [Q=1024] [milestones=50000] [--out FILE]     writes FILE, by default profiles/prm_simplify/bench.json"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from oxmpl_amd import capi, scenarios  # noqa: E402

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "prm_simplify", "bench.json")
if OUT in argv:
    argv.remove(OUT)
Q = int(argv[0]) if len(argv) > 0 else 1024
N = int(argv[1]) if len(argv) > 1 else 50000
SEED, REP, HOST_QUERIES = 42, 5, 32
SUBDIVIDE = (1, 4, 16)


def median_spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": list(v)}


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def host_route(g, m, n_queries):
    """batch_paths, the dense paths and every pair of the window on the host, one check_motion call, the DP in Python"""
    t0 = time.perf_counter()
    off, _, rows = g.batch_paths()
    answered = [q for q in range(len(off) - 1) if off[q + 1] > off[q]][:n_queries]
    dense, frm, to, spans = [], [], [], []
    for q in answered:
        p = rows[int(off[q]):int(off[q + 1])]
        t = (np.arange(1, m) / float(m))[None, :, None]
        seg = p[:-1, None, :] + (p[1:, None, :] - p[:-1, None, :]) * t          # the dense points (numpy: not the device's bits)
        d = np.concatenate([np.concatenate([p[:-1, None, :], seg], axis=1).reshape(-1, p.shape[1]), p[-1:]])
        M = len(d)
        u, v = np.triu_indices(M, 1)
        keep = u // m != (v - 1) // m
        spans.append((len(frm), int(keep.sum()), u[keep], v[keep]))
        frm.append(d[u[keep]])
        to.append(d[v[keep]])
        dense.append(d)
    ok = g.check_motion(np.concatenate(frm), np.concatenate(to)) if frm and sum(len(f) for f in frm) else np.zeros(0, dtype=bool)
    pos, checks = 0, 0
    for d, (_, n, u, v) in zip(dense, spans):
        M = len(d)
        valid = np.zeros((M, M), dtype=bool)
        iu, iv = np.triu_indices(M, 1)
        valid[iu, iv] = iu // m == (iv - 1) // m
        valid[u, v] = ok[pos:pos + n]
        pos += n
        checks += n
        dist = np.sqrt(((d[:, None, :] - d[None, :, :]) ** 2).sum(axis=2))
        cost = np.full(M, np.inf)
        cost[0] = 0.0
        for j in range(1, M):
            cand = np.where(valid[:j, j], cost[:j] + dist[:j, j], np.inf)
            cost[j] = cand.min()
    return (time.perf_counter() - t0) * 1e3, len(answered), checks


def main():
    sc = scenarios.config5()
    g = scenarios.make_prm(sc, N, seed=SEED)
    g.construct_roadmap()
    rng = np.random.default_rng(SEED)
    starts = rng.uniform(0.5, 9.5, (Q, sc["dim"]))
    goals = rng.uniform(0.5, 9.5, (Q, sc["dim"]))
    radii = np.full(Q, sc["goal_radius"])
    out = {"tool": "tools/bench_prm_simplify.py", "scene": "config 5: R^6, [0,10]^6, 32 spheres, connection radius 2.0", "seed": SEED,
           "milestones": g.sizes()[0], "queries": Q, "repetitions": REP, "statistic": "one warm-up, median of %d" % REP, "batches": {}}
    for kind, solve in (("breadth_first", lambda: g.solve_batch(starts, goals, radii)),
                        ("shortest", lambda: g.solve_batch_shortest(starts, goals, radii, weights=0))):
        solve()                                                                   # warm-up
        solve_wall = [timed(solve) for _ in range(REP)]
        status = solve()
        solve_ms = float(sum(g.batch_last_timing()["phase_ms"]))
        lens = g.batch_results()["path_len"]
        okq = status == capi.OK
        entry = {"answered": int(okq.sum()), "solve_batch_wall_ms": median_spread(solve_wall), "solve_batch_event_ms_last_run": solve_ms,
                 "raw_path_states_min_median_max": [int(lens[okq].min()), int(np.median(lens[okq])), int(lens[okq].max())] if okq.any() else None,
                 "subdivide": {}}
        for m in SUBDIVIDE:
            g.simplify_batch_paths(m)                                             # warm-up
            wall, phases = [], []
            for _ in range(REP):
                wall.append(timed(lambda: g.simplify_batch_paths(m)))
                phases.append(g.simplify_timing()["phase_ms"])
            res = g.simplify_results()
            ratio = res["simplified_cost"][okq] / res["raw_cost"][okq]
            soff = g.simplified_batch_paths()[0]
            h_ms, h_q, h_checks = host_route(g, m, HOST_QUERIES)
            total_checks = int(res["checks"].sum())
            entry["subdivide"][str(m)] = {
                "wall_ms": median_spread(wall),
                "phase_ms_median": {name: statistics.median(p[i] for p in phases)
                                    for i, name in enumerate(("upload_subdivide", "pair_matrix", "dp", "copies"))},
                "rounds": g.simplify_timing()["rounds"], "motion_checks": total_checks,
                "checks_per_second_pair_kernel": total_checks / max(1e-9, statistics.median(p[1] for p in phases) * 1e-3),
                "cost_ratio_mean": float(ratio.mean()) if okq.any() else None, "cost_ratio_worst": float(ratio.max()) if okq.any() else None,
                "simplified_states_median": float(np.median(np.diff(soff.astype(np.int64))[okq])) if okq.any() else None,
                "simplify_over_solve_batch_wall": statistics.median(wall) / statistics.median(solve_wall),
                "host_route": {"what": "batch_paths + one oxhip_prm_check_motion call over all pairs + numpy / Python DP",
                               "queries_timed": h_q, "checks_timed": h_checks, "ms_timed": h_ms,
                               "ms_extrapolated_to_the_batch_by_checks": h_ms * total_checks / max(1, h_checks)},
            }
        out["batches"][kind] = entry
    g.close()
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
