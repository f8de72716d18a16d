#!/usr/bin/env python3
"""Times oxhip_rrt_batch_revalidate_trees on the headline world (R^3, [0,10]^3, 64 spheres; P problems grown to `nodes` nodes)
after four spheres are added, against the two things a caller could do before the call existed:

  the call        wall clock and its four phases (edge checks, survival, scan, compaction + remap + skip flags), once with the
                  obstacles unchanged (every edge is checked, nothing moves) and once with the four spheres added
  deferred work   the first launch after the call rebuilds what the call dropped (fl32 shadows, cell grids): a frozen launch of
                  `--budget` iterations right after the call against the same launch once more (the second is the ordinary one)
  host loop       per problem: get_tree, check_motion on every (parent, child) pair, pruning in numpy, set_tree -- written
                  against entry points that existed before.  Timed on `--host-problems` problems and scaled to P (stated so).
  regrow          setup() in the new scene and growing every tree to the mean surviving node count

usage: tools/bench_rrt_revalidate.py [P] [nodes]
Writes profiles/rrt_revalidate/bench_rrt_revalidate.json (or --out).  No figure is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oxmpl_amd import capi, scenarios  # noqa: E402
import rrt_revalidate_helpers as rh  # noqa: E402

ADDED = (np.array([[3.0, 3.0, 3.0], [5.0, 5.0, 4.0], [2.0, 6.0, 5.0], [6.0, 2.0, 3.0]]), np.array([0.6, 0.6, 0.5, 0.7]))
PHASES = ["edge_checks", "survival", "scan", "compaction_remap_skip"]


def wall_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def frozen_launch_ms(b, budget):
    b.solve(budget, freeze=True)
    return b.last_timing()["kernel_ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("P", type=int, nargs="?", default=1024)
    ap.add_argument("nodes", type=int, nargs="?", default=10000)
    ap.add_argument("--budget", type=int, default=256)
    ap.add_argument("--host-problems", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rrt_revalidate", "bench_rrt_revalidate.json"))
    args = ap.parse_args()
    sc = scenarios.config2()
    moved = dict(sc, spheres=(np.vstack([sc["spheres"][0], ADDED[0]]), np.concatenate([sc["spheres"][1], ADDED[1]])))
    P = args.P

    def grown():
        b = scenarios.make_batch(sc, P, args.nodes, False, 42, 0, 0, capi.KERNEL_AUTO)
        b.solve(1 << 30)
        return b
    a = grown()
    nodes = a.counts()["nodes"].copy()
    frozen_launch_ms(a, args.budget)
    before = frozen_launch_ms(a, args.budget)   # (every tree is full and says so: such a launch may have nothing to do)
    # unchanged obstacles (also the warm-up: workspace allocation, code loading)
    a.revalidate_trees()
    frozen_launch_ms(a, args.budget)
    t_same, r_same = wall_ms(a.revalidate_trees)
    assert not r_same["n_removed"].any()
    ph_same = a.revalidate_last_timing()["phase_ms"].tolist()
    after_same = frozen_launch_ms(a, args.budget)
    again_same = frozen_launch_ms(a, args.budget)
    # four spheres arrive
    a.set_spheres(*moved["spheres"])
    t_moved, r_moved = wall_ms(a.revalidate_trees)
    ph_moved = a.revalidate_last_timing()["phase_ms"].tolist()
    after_moved = frozen_launch_ms(a, args.budget)
    again_moved = frozen_launch_ms(a, args.budget)
    kept = a.counts()["nodes"].copy()
    # the host loop, on a batch grown the same way
    b = grown()
    b.set_spheres(*moved["spheres"])
    hp = min(args.host_problems, P)

    def host_loop():
        for p in range(hp):
            s, par = b.tree(p)
            edge_ok = np.ones(len(par), dtype=bool)
            edge_ok[1:] = b.check_motion(*rh.edge_rows(s, par))
            pr = rh.prune(s, par, edge_ok)
            b.set_tree(p, pr["states"], pr["parents"])
    t_host, _ = wall_ms(host_loop)
    assert np.array_equal(b.counts()["nodes"][:hp], kept[:hp])
    b.close()
    # setup + regrow in the new scene
    target = max(2, int(round(float(kept.mean()))))
    c = scenarios.make_batch(moved, P, target, False, 42, 0, 0, capi.KERNEL_AUTO)

    def regrow():
        c.setup(moved["start"], moved["goal_centre"], moved["goal_radius"])
        c.solve(1 << 30)
    regrow()
    t_regrow, _ = wall_ms(regrow)
    regrow_kernel = c.last_timing()["kernel_ms"]
    out = dict(tool="tools/bench_rrt_revalidate.py", problems=P, max_nodes=args.nodes, nodes_before=int(nodes.sum()), nodes_after=int(kept.sum()),
               removed=int(r_moved["n_removed"].sum()), goals_lost=int(r_moved["goal_lost"].sum()), added_spheres=len(ADDED[1]),
               unchanged=dict(wall_ms=round(t_same, 4), phase_ms=dict(zip(PHASES, [round(v, 4) for v in ph_same]))),
               moved=dict(wall_ms=round(t_moved, 4), phase_ms=dict(zip(PHASES, [round(v, 4) for v in ph_moved]))),
               deferred=dict(budget=args.budget, launch_before_any_call_ms=round(before, 4), first_launch_after_unchanged_ms=round(after_same, 4),
                             second_launch_after_unchanged_ms=round(again_same, 4), first_launch_after_moved_ms=round(after_moved, 4),
                             second_launch_after_moved_ms=round(again_moved, 4)),
               host_loop=dict(problems_timed=hp, wall_ms=round(t_host, 3), scaled_to_all_problems_ms=round(t_host * P / hp, 3)),
               regrow=dict(target_nodes=target, setup_and_solve_wall_ms=round(t_regrow, 4), last_launch_kernel_ms=round(regrow_kernel, 4)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:   # a line per top-level key
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(out[k], sort_keys=True)) for k in sorted(out)) + "\n}\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
