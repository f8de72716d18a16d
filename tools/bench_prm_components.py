#!/usr/bin/env python3
"""Times oxhip_prm_components and oxhip_prm_prune on the config-5 roadmap (R^6, 50,000 milestones, 32 hyperspheres, r = 2) after
the scene of tools/bench_prm_grow.py moved (four hyperspheres added) and the roadmap was re-checked.

Each repeat: construct in the old scene, set the moved scene's spheres, revalidate; then
  (a) components() on the re-checked roadmap, by its own HIP events (the labels are computed: the re-check dropped the kept ones);
  (b) what a user did before: get_roadmap (the device-to-host copy of the whole CSR and the states) plus a union-find on the
      host in numpy (minimum-label propagation with pointer jumping), by the wall clock; its labels must equal (a)'s;
  (c) prune(invalid=True), by its own HIP events and by the wall clock;
  (d) for context, the revalidate before and a grow back to `milestones` afterwards, by their own events.
One warm-up repeat, then the best and the median of `--repeats`.

Writes profiles/prm_components/bench.json (or --out).  No figure is asserted."""
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
CC_PHASES = ["init_hook", "flatten", "sizes_summary", "copies"]
PRUNE_PHASES = ["masks", "components", "scans", "move_entries", "move_states"]
REVAL_PHASES = ["milestone_validity", "pair_emission", "edge_checks", "compaction"]
GROW_PHASES = ["liveness_mask", "keys_from_csr", "sampling", "pair_search_filter", "edge_checks", "sort_csr"]


def best_median(values):
    return dict(best=round(min(values), 5), median=round(statistics.median(values), 5))


def wall_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def host_labels(offsets, nbrs):
    """label[i] = the lowest index of i's component: every milestone takes the smallest label among itself and its neighbours,
    then every label jumps to its own label, until nothing changes"""
    n = len(offsets) - 1
    rows = np.repeat(np.arange(n), np.diff(offsets.astype(np.int64)))
    nb = nbrs.astype(np.int64)
    label = np.arange(n)
    rounds = 0
    while True:
        rounds += 1
        new = label.copy()
        np.minimum.at(new, rows, label[nb])
        while True:
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, label):
            return label, rounds
        label = new


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("milestones", type=int, nargs="?", default=50000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prm_components", "bench.json"))
    args = ap.parse_args()
    sc = scenarios.config5()
    moved = dict(sc, spheres=(np.vstack([sc["spheres"][0], ADDED[0]]), np.concatenate([sc["spheres"][1], ADDED[1]])))
    g = scenarios.make_prm(sc, args.milestones)
    rec = dict(cc=[], cc_wall=[], host_copy=[], host_uf=[], prune=[], prune_wall=[], reval=[], grow=[])
    facts = {}
    for rep in range(args.repeats + 1):
        g.set_spheres(*sc["spheres"])
        g.setup(sc["start"], sc["goal_centre"], sc["goal_radius"])
        g.construct_roadmap()
        built = g.sizes()
        g.set_spheres(*moved["spheres"])
        valid, removed = g.revalidate()
        ph_reval = g.revalidate_last_timing()["phase_ms"]
        dead = int(np.count_nonzero(~valid))
        rechecked = g.sizes()
        t_cc, (label, size, n_comp, largest_label, largest_size) = wall_ms(g.components)
        cc = g.components_timing()
        t_copy, (states, offsets, nbrs) = wall_ms(g.roadmap)
        t_uf, (h_label, h_rounds) = wall_ms(lambda: host_labels(offsets, nbrs))
        if not np.array_equal(h_label, label.astype(np.int64)):
            raise SystemExit("the host union-find and oxhip_prm_components disagree")
        t_prune, (new_index, n_kept, removed_by_prune) = wall_ms(lambda: g.prune(invalid=True))
        ph_prune = g.prune_timing()["phase_ms"]
        pruned = g.sizes()
        added, drawn = g.grow(dead)
        ph_grow = g.grow_timing()["phase_ms"]
        facts = dict(milestones_built=built[0], edge_entries_built=built[1], invalid_milestones=dead, removed_entries_recheck=int(removed),
                     edge_entries_rechecked=rechecked[1], n_components=n_comp, largest_component=largest_size, largest_label=largest_label,
                     component_launches=cc["launches"], host_rounds=h_rounds, milestones_pruned=pruned[0], edge_entries_pruned=pruned[1],
                     removed_entries_prune=int(removed_by_prune), milestones_added=added, milestones_grown=g.sizes()[0],
                     edge_entries_grown=g.sizes()[1])
        if n_kept != built[0] - dead or int(np.count_nonzero(new_index < 0)) != dead:
            raise SystemExit("prune(invalid=True) did not drop exactly the invalid milestones")
        if rep == 0:
            continue                                       # warm-up: first-use allocations, code loading
        rec["cc"].append(cc["phase_ms"]); rec["cc_wall"].append(t_cc)
        rec["host_copy"].append(t_copy); rec["host_uf"].append(t_uf)
        rec["prune"].append(ph_prune); rec["prune_wall"].append(t_prune)
        rec["reval"].append(ph_reval); rec["grow"].append(ph_grow)

    def phases(rows, names):
        return {nm: best_median([r[i] for r in rows]) for i, nm in enumerate(names)}

    def timed(rows, names, wall=None):
        d = dict(event_ms=best_median([sum(r) for r in rows]), phase_ms=phases(rows, names))
        if wall is not None:
            d["wall_ms"] = best_median(wall)
        return d

    out = dict(tool="tools/bench_prm_components.py", repeats=args.repeats, added_spheres=len(ADDED[1]), **facts,
               components=timed(rec["cc"], CC_PHASES, rec["cc_wall"]),
               host_way=dict(get_roadmap_wall_ms=best_median(rec["host_copy"]), union_find_wall_ms=best_median(rec["host_uf"]),
                             wall_ms=best_median([a + b for a, b in zip(rec["host_copy"], rec["host_uf"])])),
               prune_invalid=timed(rec["prune"], PRUNE_PHASES, rec["prune_wall"]),
               revalidate=timed(rec["reval"], REVAL_PHASES), grow=timed(rec["grow"], GROW_PHASES))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:   # a line per top-level key
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(out[k], sort_keys=True)) for k in sorted(out)) + "\n}\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
