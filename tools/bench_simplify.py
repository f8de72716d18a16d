#!/usr/bin/env python3
"""The solution paths of a whole batch on BASELINE.json's config 2 (R^3, 64 spheres), [P] problems
solved with stop_at_goal:
  (a) the loop of oxhip_rrt_batch_get_path over all problems (one tree copy and a host walk per problem);
  (b) oxhip_rrt_batch_extract_paths + oxhip_rrt_batch_get_paths (chain walk on the device, one copy);
  (c) oxhip_rrt_batch_simplify_paths at full span, split per kernel by HIP events (pair matrix, DP).
(a) and (b) alternate in the same process; wall clock around calls that end in a synchronise, best of 3 after a warm-up, with
the spread.  Refuses to print unless (a) and (b) return identical rows.  The CPU figure is the oracle's C check_motion driven
from Python over the pairs of the first problems, one ctypes call per pair, single thread: a measured rate of exactly that.

Usage: bench_simplify.py [P=1024] [--out FILE]"""
import ctypes as C
import json
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
P = int(argv[0]) if len(argv) > 0 else 1024
SEED, REP, CAP = 42, 3, 4096
ORACLE_PROBLEMS = 32
L = capi.lib()
_dp, _u32p, _u64p = (C.POINTER(t) for t in (C.c_double, C.c_uint32, C.c_uint64))


def loop(g):
    buf = np.zeros((CAP, g.dim))
    ln = C.c_uint32()
    paths = []
    t0 = time.perf_counter()
    for p in range(g.n_problems):
        st = L.oxhip_rrt_batch_get_path(g._h, p, buf.ctypes.data_as(_dp), CAP, C.byref(ln))
        if st != capi.OK:
            raise SystemExit("get_path failed: %d" % st)
        paths.append(buf[:ln.value].copy())
    return (time.perf_counter() - t0) * 1e3, paths


def batched(g):
    off, total = np.zeros(g.n_problems + 1, dtype=np.uint64), C.c_uint64()
    rows = np.zeros((g.n_problems * 128, g.dim))
    t0 = time.perf_counter()
    st = L.oxhip_rrt_batch_extract_paths(g._h)
    st2 = L.oxhip_rrt_batch_get_paths(g._h, off.ctypes.data_as(_u64p), rows.ctypes.data_as(_dp), len(rows), C.byref(total))
    wall = (time.perf_counter() - t0) * 1e3
    if st != capi.OK or st2 != capi.OK:
        raise SystemExit("extract / get_paths failed: %d %d %s" % (st, st2, L.oxhip_last_error_string().decode()))
    return wall, [rows[int(off[p]):int(off[p + 1])].copy() for p in range(g.n_problems)], g.paths_last_timing()["extract_ms"]


def simplify(g):
    t0 = time.perf_counter()
    g.simplify_paths(0)
    wall = (time.perf_counter() - t0) * 1e3
    return wall, g.paths_last_timing()


def spread(v):
    return {"ms": v, "best": min(v), "spread": max(v) - min(v)}


def oracle_rate(paths):
    from oracle import oracle_py as orc
    sc = scenarios.config2()
    o = orc.OracleRRT(sc["dim"], sc["bounds"], sc["max_distance"], sc["goal_bias"], sc["lvs_fraction"], 10000, True, SEED, 0)
    o.set_spheres(*sc["spheres"])
    o.setup(sc["start"], sc["goal_centre"], sc["goal_radius"])
    pairs = [(p[i], p[j]) for p in paths[:ORACLE_PROBLEMS] for i in range(len(p)) for j in range(i + 2, len(p))]
    t0 = time.perf_counter()
    ok = sum(o.check_motion(a, b) for a, b in pairs)
    dt = time.perf_counter() - t0
    return {"what": "oracle C check_motion, one ctypes call per pair from Python, one thread", "pairs": len(pairs), "valid": int(ok),
            "seconds": dt, "checks_per_second": len(pairs) / dt}


def main():
    sc = scenarios.config2()
    g = scenarios.make_batch(sc, P, 10000, True, SEED)
    status = g.solve(10 ** 6)
    counts = g.counts()
    loop(g), batched(g), simplify(g)                      # warm-up of every call that is timed
    a, b = [], []
    for _ in range(REP):                                  # alternating
        a.append(loop(g))
        b.append(batched(g))
    for run in a[1:] + b:
        if any(x.shape != y.shape or not np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(run[1], a[0][1])):
            raise SystemExit("the loop and the batch disagree -- nothing to report")
    c = [simplify(g) for _ in range(REP)]
    off, rows, idx, raw, simp, checks = g.simplified_paths()
    valid_bits = sum(int(g.path_valid_matrix(p).sum()) - (len(a[0][1][p]) - 1) for p in range(min(P, ORACLE_PROBLEMS)) if len(a[0][1][p]))
    lens = np.array([len(p) for p in a[0][1]])
    solved = lens > 0
    aw, bw = [r[0] for r in a], [r[0] for r in b]
    out = {
        "tool": "tools/bench_simplify.py", "scene": "config 2: R^3, [0,10]^3, 64 spheres, stop_at_goal, max_nodes 10000", "seed": SEED,
        "problems": P, "solved": int(np.sum(status == capi.OK)), "repetitions": REP,
        "tree_nodes_min_median_max": [int(np.min(counts["nodes"])), int(np.median(counts["nodes"])), int(np.max(counts["nodes"]))],
        "raw_path_states_min_median_max": [int(lens[solved].min()), int(np.median(lens[solved])), int(lens[solved].max())],
        "simplified_path_states_min_median_max": [int(v) for v in (np.diff(off)[solved].min(), np.median(np.diff(off)[solved]),
                                                                      np.diff(off)[solved].max())],
        "mean_cost_ratio": float(np.mean(simp[solved] / raw[solved])),
        "motion_checks_total": int(checks.sum()), "motion_checks_per_path_median": int(np.median(checks[solved])),
        "valid_share_first_problems": valid_bits / max(1, int(checks[:ORACLE_PROBLEMS].sum())),
        "a_loop_of_get_path": dict(spread(aw), per_problem_ms=min(aw) / P),
        "b_extract_paths_plus_get_paths": dict(spread(bw), per_problem_ms=min(bw) / P, extract_kernels_ms=spread([r[2] for r in b])),
        "b_beats_a_by_more_than_a_spread": bool(min(aw) - min(bw) > max(aw) - min(aw)),
        "speedup_wall_a_over_b": min(aw) / min(bw),
        "c_simplify_paths": {"wall": spread([r[0] for r in c]), "pairs_kernel": spread([r[1]["pairs_ms"] for r in c]),
                             "dp_kernel": spread([r[1]["dp_ms"] for r in c]), "rounds": c[0][1]["rounds"],
                             "checks_per_second_pairs_kernel": float(checks.sum()) / (min(r[1]["pairs_ms"] for r in c) * 1e-3)},
        "identical_rows": True,
        "cpu": oracle_rate(a[0][1]),
        "not_measured": ["hardware counters", "other dealings of the pair matrix (i-major, one wave per motion)", "SE(2) / SE(3)"],
    }
    g.close()
    text = json.dumps(out, indent=1)
    print(text)
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
