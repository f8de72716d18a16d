#!/usr/bin/env python3
"""Many queries on one PRM roadmap: the loop of set_problem + solve (query kernel, flag copy, host
breadth-first search; one query per call) next to one oxhip_prm_solve_batch + oxhip_prm_batch_get_paths (flags, search and
path extraction on the device), on
  * BASELINE.json configs[4]: R^6, 32 hyperspheres, connection radius 2, [milestones] milestones, [Q] seeded queries;
  * the SO(3) fixture (one 44.9 degree cone, radius 0.5) at 16,384 milestones, Q / 4 seeded queries.
Wall clock and HIP events, best of 3 after a warm-up.  Refuses to print unless both ways returned identical statuses and paths.

Usage: bench_prm_queries.py [Q=1024] [milestones=50000] [--out FILE]"""
import ctypes as C
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from oxmpl_amd import capi, scenarios  # noqa: E402

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
if OUT in argv:
    argv.remove(OUT)
Q = int(argv[0]) if len(argv) > 0 else 1024
N = int(argv[1]) if len(argv) > 1 else 50000
SEED, REP, CAP_ROWS = 20261016, 3, 4096
L = capi.lib()
_dp, _u32p, _i32p, _u64p = (C.POINTER(t) for t in (C.c_double, C.c_uint32, C.c_int32, C.c_uint64))


def loop(g, starts, goals, radii):
    """the only way before the batch: one set_problem + solve per query (one call each, the path buffer large enough)"""
    buf = np.zeros((CAP_ROWS, g.dim))
    ln, ms = C.c_uint32(), np.zeros(6)
    status, paths, kernel_ms, bfs_ms = [], [], 0.0, 0.0
    t0 = time.perf_counter()
    for q in range(len(radii)):
        L.oxhip_prm_set_problem(g._h, starts[q].ctypes.data_as(_dp), goals[q].ctypes.data_as(_dp), radii[q])
        st = L.oxhip_prm_solve(g._h, 0.0, buf.ctypes.data_as(_dp), CAP_ROWS, C.byref(ln))
        status.append(st)
        paths.append(buf[:ln.value].copy())
        L.oxhip_prm_last_timing(g._h, ms.ctypes.data_as(_dp), None, None)
        kernel_ms += ms[4]
        if st != capi.ERR_INVALID_START_STATE:          # (an invalid start returns before the search: its slot holds the previous query's)
            bfs_ms += ms[5]
    return (time.perf_counter() - t0) * 1e3, np.array(status, dtype=np.int32), paths, kernel_ms, bfs_ms


def batch(g, starts, goals, radii):
    q = len(radii)
    status, off, total = np.zeros(q, dtype=np.int32), np.zeros(q + 1, dtype=np.uint64), C.c_uint64()
    nodes, rows = np.zeros(q * 64, dtype=np.uint32), np.zeros((q * 64, g.dim))
    t0 = time.perf_counter()
    st = L.oxhip_prm_solve_batch(g._h, q, starts.ctypes.data_as(_dp), goals.ctypes.data_as(_dp), radii.ctypes.data_as(_dp), 0.0, 0,
                                 status.ctypes.data_as(_i32p))
    st2 = L.oxhip_prm_batch_get_paths(g._h, off.ctypes.data_as(_u64p), nodes.ctypes.data_as(_u32p), rows.ctypes.data_as(_dp), len(nodes),
                                      C.byref(total))
    wall = (time.perf_counter() - t0) * 1e3
    if st != capi.OK or st2 != capi.OK:
        raise SystemExit("batch failed: %d %d %s" % (st, st2, L.oxhip_last_error_string().decode()))
    return wall, status, [rows[int(off[k]):int(off[k + 1])].copy() for k in range(q)], g.batch_last_timing()


def measure(name, g, starts, goals, radii):
    starts, goals, radii = (np.ascontiguousarray(a, dtype=np.float64) for a in (starts, goals, radii))
    n, entries, _ = g.sizes()
    loop(g, starts[:8], goals[:8], radii[:8])           # warm-up of both ways (the first solve also copies the roadmap to the host)
    batch(g, starts, goals, radii)
    loops = [loop(g, starts, goals, radii) for _ in range(REP)]
    batches = [batch(g, starts, goals, radii) for _ in range(REP)]
    ref_status, ref_paths = loops[0][1], loops[0][2]
    for run in loops[1:] + batches:
        if not np.array_equal(run[1], ref_status) or any(a.shape != b.shape or not np.array_equal(a.view(np.uint64), b.view(np.uint64))
                                                         for a, b in zip(run[2], ref_paths)):
            raise SystemExit("%s: the loop and the batch disagree -- nothing to report" % name)
    lw, bw = [r[0] for r in loops], [r[0] for r in batches]
    best_l, best_b = min(range(REP), key=lambda i: lw[i]), min(range(REP), key=lambda i: bw[i])
    t = batches[best_b][3]
    lens = [len(p) for p in ref_paths if len(p)]
    q = len(radii)
    return {
        "roadmap": name, "milestones": n, "edge_entries": entries, "mean_degree": entries / n, "queries": q,
        "solved": int(np.sum(ref_status == capi.OK)), "no_solution": int(np.sum(ref_status == capi.ERR_NO_SOLUTION_FOUND)),
        "invalid_start": int(np.sum(ref_status == capi.ERR_INVALID_START_STATE)),
        "path_states_min_median_max": [int(min(lens)), int(np.median(lens)), int(max(lens))] if lens else None,
        "loop": {"wall_ms": lw, "wall_ms_best": min(lw), "wall_ms_spread": max(lw) - min(lw), "per_query_ms": min(lw) / q,
                 "query_kernel_ms_sum": loops[best_l][3], "host_bfs_ms_sum": loops[best_l][4]},
        "batch": {"wall_ms": bw, "wall_ms_best": min(bw), "wall_ms_spread": max(bw) - min(bw), "per_query_ms": min(bw) / q,
                  "phase_ms": dict(zip(("flags", "search", "paths", "copies"), t["phase_ms"])), "rounds": t["rounds"]},
        "speedup_wall": min(lw) / min(bw),
        "batch_beats_loop_by_more_than_its_spread": bool(min(lw) - min(bw) > max(lw) - min(lw)),
        "identical_statuses_and_paths": True,
    }


def main():
    out = {"tool": "tools/bench_prm_queries.py", "seed": SEED, "repetitions": REP, "rows": []}
    sc = scenarios.config5()
    g = scenarios.make_prm(sc, N)
    g.construct_roadmap()
    rng = np.random.default_rng(SEED)
    starts = rng.uniform(0.0, 10.0, size=(Q, 6))
    goals = rng.uniform(0.0, 10.0, size=(Q, 6))
    radii = rng.uniform(1.5, 2.5, size=Q)
    out["rows"].append(measure("config 5: R^6, 32 hyperspheres, radius 2", g, starts, goals, radii))
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
    out["rows"].append(measure("SO(3) fixture: one 44.9 degree cone, radius 0.5", g, starts, goals, radii))
    g.close()
    text = json.dumps(out, indent=1)
    print(text)
    if OUT:
        with open(OUT, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
