#!/usr/bin/env python3
"""Times oxhip_prm_revalidate and oxhip_prm_set_roadmap on the config-5 roadmap (R^6, 50,000 milestones, 32 hyperspheres, r = 2)
against the handle's own construct_roadmap.  One process, the candidates alternating, one warm-up round and
then `--rounds` timed ones; every figure is reported as best / median / worst so that the spread shows.

  moved scene      four hyperspheres are added.  (a) a handle planted with the old roadmap re-checks it (revalidate);
                   (b) a handle in the same new scene runs setup + construct_roadmap.  Wall clock around each call, and the
                   phases each reports (oxhip_prm_revalidate_last_timing, oxhip_prm_last_timing).
  same motions     revalidate in the UNCHANGED scene checks the roadmap's edges, which are construction's candidate pairs less the
                   few that failed: its edge phase against construction's edge phase, on the same motions.
  planting         set_roadmap (upload, device checks, shadow) against construct_roadmap, wall clock.

Writes profiles/prm_revalidate/bench_prm_revalidate.json (or --out).  No figure is asserted."""
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


def spread(values):
    return dict(best=round(min(values), 5), median=round(statistics.median(values), 5), worst=round(max(values), 5))


def wall_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--milestones", type=int, default=50000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prm_revalidate", "bench_prm_revalidate.json"))
    args = ap.parse_args()
    sc = scenarios.config5()
    moved = dict(sc, spheres=(np.vstack([sc["spheres"][0], ADDED[0]]), np.concatenate([sc["spheres"][1], ADDED[1]])))
    base = scenarios.make_prm(sc, args.milestones)
    base.construct_roadmap()
    rm = base.roadmap()
    n, entries, _ = base.sizes()
    g_old = scenarios.make_prm(sc, args.milestones)       # unchanged scene: plant, revalidate; setup, construct
    g_new = scenarios.make_prm(moved, args.milestones)    # moved scene: the same
    g_ctor = scenarios.make_prm(moved, args.milestones)
    rec = dict(reval_moved=[], reval_moved_phases=[], ctor_moved=[], ctor_moved_phases=[], reval_same=[], reval_same_phases=[],
               ctor_same=[], ctor_same_phases=[], plant=[])
    removed = invalid = None
    for rnd in range(args.rounds + 1):
        t_plant, _ = wall_ms(lambda: g_new.set_roadmap(*rm))
        t_rev, (valid, removed) = wall_ms(g_new.revalidate)
        invalid = int(np.count_nonzero(~valid))
        ph_rev = g_new.revalidate_last_timing()["phase_ms"]

        def rebuild(g, s):
            g.setup(s["start"], s["goal_centre"], s["goal_radius"])
            g.construct_roadmap()
        t_ctor, _ = wall_ms(lambda: rebuild(g_ctor, moved))
        ph_ctor = g_ctor.last_timing()["phase_ms"][:4]
        g_old.set_roadmap(*rm)
        t_rev_same, (valid_same, removed_same) = wall_ms(g_old.revalidate)
        assert valid_same.all() and removed_same == 0
        ph_rev_same = g_old.revalidate_last_timing()["phase_ms"]
        t_ctor_same, _ = wall_ms(lambda: rebuild(g_old, sc))
        ph_ctor_same = g_old.last_timing()["phase_ms"][:4]
        cand_same = g_old.last_timing()["candidates"]
        if rnd == 0:
            continue                                       # warm-up: first-use allocations, code loading
        rec["plant"].append(t_plant)
        rec["reval_moved"].append(t_rev); rec["reval_moved_phases"].append(ph_rev)
        rec["ctor_moved"].append(t_ctor); rec["ctor_moved_phases"].append(ph_ctor)
        rec["reval_same"].append(t_rev_same); rec["reval_same_phases"].append(ph_rev_same)
        rec["ctor_same"].append(t_ctor_same); rec["ctor_same_phases"].append(ph_ctor_same)

    def phases(rows, names):
        return {nm: spread([r[i] for r in rows]) for i, nm in enumerate(names)}

    rv_names = ["milestone_validity", "pair_emission", "edge_checks", "compaction"]
    ct_names = ["sampling", "pair_search", "edge_checks", "sort_csr"]
    out = dict(tool="tools/bench_prm_revalidate.py", milestones=int(n), edge_entries=int(entries), rounds=args.rounds,
               added_spheres=len(ADDED[1]), invalid_milestones=invalid, removed_entries=int(removed),
               moved_scene=dict(revalidate_wall_ms=spread(rec["reval_moved"]), revalidate_phase_ms=phases(rec["reval_moved_phases"], rv_names),
                                setup_construct_wall_ms=spread(rec["ctor_moved"]), construct_phase_ms=phases(rec["ctor_moved_phases"], ct_names)),
               same_motions=dict(motions_rechecked=int(entries) // 2, construction_candidates=int(cand_same),
                                 revalidate_wall_ms=spread(rec["reval_same"]), revalidate_phase_ms=phases(rec["reval_same_phases"], rv_names),
                                 setup_construct_wall_ms=spread(rec["ctor_same"]), construct_phase_ms=phases(rec["ctor_same_phases"], ct_names)),
               planting=dict(set_roadmap_wall_ms=spread(rec["plant"]), setup_construct_wall_ms=spread(rec["ctor_same"])))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:   # a line per top-level key
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(out[k], sort_keys=True)) for k in sorted(out)) + "\n}\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
