#!/usr/bin/env python3
"""Times oxhip_prm_grow_roadmap on the config-5 roadmap (R^6, 50,000 milestones, 32 hyperspheres, r = 2) after the scene of
tools/bench_prm_revalidate.py moved (four hyperspheres added), against what a user did before: setup + construct_roadmap in the
new scene.

Each repeat: construct in the old scene, set the moved scene's spheres, revalidate, then grow by the number of milestones the
re-check found invalid -- back to `milestones` live ones.  The grow is timed by its own HIP events (the six phases of
oxhip_prm_grow_last_timing, and their sum) and by the wall clock around the call; the rebuild, on a second handle and alternating
with it, by construct's events and the wall clock around setup + construct_roadmap.  One warm-up repeat, then the best and the
median of `--repeats`.

Writes profiles/prm_grow/bench_prm_grow.json (or --out).  No figure is asserted."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oxmpl_amd import scenarios  # noqa: E402

ADDED = ([[3.0, 7.0, 5.0, 5.0, 3.0, 7.0], [7.0, 3.0, 5.0, 5.0, 7.0, 3.0], [5.0, 5.0, 2.5, 7.5, 5.0, 5.0], [6.5, 6.5, 6.5, 3.5, 3.5, 3.5]],
         [1.6, 1.6, 1.4, 1.2])
GROW_PHASES = ["liveness_mask", "keys_from_csr", "sampling", "pair_search_filter", "edge_checks", "sort_csr"]
CTOR_PHASES = ["sampling", "pair_search", "edge_checks", "sort_csr"]


def best_median(values):
    return dict(best=round(min(values), 5), median=round(statistics.median(values), 5))


def wall_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("milestones", type=int, nargs="?", default=50000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prm_grow", "bench_prm_grow.json"))
    args = ap.parse_args()
    sc = scenarios.config5()
    moved = dict(sc, spheres=(np.vstack([sc["spheres"][0], ADDED[0]]), np.concatenate([sc["spheres"][1], ADDED[1]])))
    g = scenarios.make_prm(sc, args.milestones)           # constructs in the old scene, re-checks and grows in the moved one
    g_ctor = scenarios.make_prm(moved, args.milestones)   # the moved scene from scratch
    rec = dict(grow_wall=[], grow_phases=[], ctor_wall=[], ctor_phases=[], reval_wall=[])
    facts = {}
    for rep in range(args.repeats + 1):
        g.set_spheres(*sc["spheres"])
        g.setup(sc["start"], sc["goal_centre"], sc["goal_radius"])
        g.construct_roadmap()
        built = g.sizes()
        g.set_spheres(*moved["spheres"])
        t_rev, (valid, removed) = wall_ms(g.revalidate)
        dead = int(np.count_nonzero(~valid))
        entries_rechecked = g.sizes()[1]
        t_grow, (added, drawn) = wall_ms(lambda: g.grow(dead))
        ph_grow = g.grow_timing()["phase_ms"]

        def rebuild():
            g_ctor.setup(moved["start"], moved["goal_centre"], moved["goal_radius"])
            g_ctor.construct_roadmap()
        t_ctor, _ = wall_ms(rebuild)
        ph_ctor = g_ctor.last_timing()["phase_ms"][:4]
        facts = dict(milestones_built=built[0], edge_entries_built=built[1], invalid_milestones=dead, removed_entries=int(removed),
                     edge_entries_rechecked=entries_rechecked, milestones_added=added, samples_drawn=drawn,
                     milestones_grown=g.sizes()[0], edge_entries_grown=g.sizes()[1], edge_entries_rebuilt=g_ctor.sizes()[1])
        if rep == 0:
            continue                                       # warm-up: first-use allocations, code loading
        rec["reval_wall"].append(t_rev)
        rec["grow_wall"].append(t_grow); rec["grow_phases"].append(ph_grow)
        rec["ctor_wall"].append(t_ctor); rec["ctor_phases"].append(ph_ctor)

    def phases(rows, names):
        return {nm: best_median([r[i] for r in rows]) for i, nm in enumerate(names)}

    out = dict(tool="tools/bench_prm_grow.py", repeats=args.repeats, added_spheres=len(ADDED[1]), **facts,
               grow=dict(event_ms=best_median([sum(r) for r in rec["grow_phases"]]), wall_ms=best_median(rec["grow_wall"]),
                         phase_ms=phases(rec["grow_phases"], GROW_PHASES)),
               revalidate_wall_ms=best_median(rec["reval_wall"]),
               setup_construct=dict(event_ms=best_median([sum(r) for r in rec["ctor_phases"]]), wall_ms=best_median(rec["ctor_wall"]),
                                    phase_ms=phases(rec["ctor_phases"], CTOR_PHASES)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:   # a line per top-level key
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(out[k], sort_keys=True)) for k in sorted(out)) + "\n}\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
