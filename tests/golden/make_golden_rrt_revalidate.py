#!/usr/bin/env python3
"""Generates tests/golden/rrt_revalidate.json: planted RRT trees re-checked after obstacles were added
(oxhip_rrt_batch_revalidate_trees), by a pure-Python restatement on top of the existing restatements of
check_motion (make_golden.py for R^n, make_golden_so3.py for SO(3)).

The semantics are the build's own (the reference has no such call): edge_ok[i] = check_motion(from = node parent[i], to = node i)
in the NEW scene, the direction the planner checked the edge in; node 0 stays, node i stays iff edge_ok[i] and its parent stays;
survivors keep their order, parents are remapped; a node carries the skip flag iff a SURVIVING node of lower index has equal
coordinates; goal_node is the lowest surviving index >= 1 inside the goal ball, -1 if none.

The trees and obstacles come from tests/rrt_revalidate_helpers.py (planted_scenes: three trees per scene in one obstacle field);
what is computed HERE -- with loops of this file's own, not the helper's -- is everything that follows from them.  Per tree: the
indices whose edge fails, the indices inside the goal ball, n, n_removed, goal_node before and after, CRC-32s of new_index, the
remapped parents and the skip flags, and those three arrays in full where the tree is small.  Scenes marked partial are asserted
to lose some but not all nodes of tree C (0 < removed < n - 1), tree A none and tree B all but the root.

Run:  python tests/golden/make_golden_rrt_revalidate.py      (about a minute)
"""
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import make_golden_so3 as g3  # noqa: E402
import rrt_revalidate_helpers as rh  # noqa: E402

FRACTION = 0.05
FULL_BELOW = 100   # trees smaller than this are stored in full


def crc(arr, dtype):
    return "%08x" % (zlib.crc32(np.ascontiguousarray(arr, dtype=dtype).tobytes()) & 0xFFFFFFFF)


def checkers(scene):
    """(check_motion(a, b), satisfied(state, goal)) of the scene's space, from the restatements"""
    if scene.get("so3"):
        cones = g3.Cones([(list(c), r) for c, r in scene["spheres"]])
        return (lambda a, b: g3.check_motion(cones, FRACTION, list(a), list(b))), (lambda s, g: g3.distance(list(s), list(g[0])) <= g[1])
    dim = scene["dim"]
    field = mg.Field(dim, [(list(c), r) for c, r in scene["spheres"]], [(list(lo), list(hi)) for lo, hi in scene["boxes"]])
    bounds = [(rh.BOUNDS_LO, rh.BOUNDS_HI)] * dim
    return (lambda a, b: mg.check_motion(field, bounds, FRACTION, list(a), list(b))), (lambda s, g: mg.distance(list(s), list(g[0])) <= g[1])


def recheck(states, parents, check_motion, satisfied, goal):
    """the plain semantics, from scratch"""
    n = len(parents)
    edge_ok = [True] + [bool(check_motion(states[parents[i]], states[i])) for i in range(1, n)]
    alive = [True] * n
    for i in range(1, n):
        alive[i] = edge_ok[i] and alive[parents[i]]
    new_index, k = [], 0
    for i in range(n):
        new_index.append(k if alive[i] else -1)
        k += 1 if alive[i] else 0
    kept = [i for i in range(n) if alive[i]]
    new_parents = [-1 if parents[i] < 0 else new_index[parents[i]] for i in kept]
    skip = []
    for a, i in enumerate(kept):
        skip.append(1 if any(all(float(x) == float(y) for x, y in zip(states[i], states[j])) for j in kept[:a]) else 0)
    sat = [bool(satisfied(states[i], goal)) for i in range(n)]
    before = next((i for i in range(1, n) if sat[i]), -1)
    after = next((a for a, i in enumerate(kept) if a >= 1 and sat[i]), -1)
    rec = dict(n=n, failed_edges=[i for i in range(n) if not edge_ok[i]], in_goal=[i for i in range(n) if sat[i]],
               n_removed=n - len(kept), goal_before=before, goal_after=after, new_index_crc=crc(new_index, np.int32),
               parents_crc=crc(new_parents, np.int32), skip_crc=crc(skip, np.uint8), states_crc=crc(states, np.float64),
               skip_set=[a for a, f in enumerate(skip) if f])
    if n < FULL_BELOW:
        rec.update(new_index=new_index, parents=new_parents, skip=skip)
    return rec


def main():
    out = {"_generator": "tests/golden/make_golden_rrt_revalidate.py", "fraction": FRACTION}
    for name, (build, partial) in rh.planted_scenes().items():
        scene = build()
        scene["so3"] = name.startswith("so3")
        cm, sat = checkers(scene)
        trees = [recheck(s, [int(v) for v in p], cm, sat, g) for (s, p), g in zip(scene["trees"], scene["goals"])]
        n = trees[2]["n"]
        assert trees[0]["n_removed"] == 0, (name, "tree A lost nodes", trees[0]["failed_edges"])
        assert trees[1]["n_removed"] == n - 1, (name, "tree B kept nodes")
        if partial:
            assert 0 < trees[2]["n_removed"] < n - 1, (name, trees[2]["n_removed"], n)
        print(name, "n", n, "removed", [t["n_removed"] for t in trees], "goal", trees[2]["goal_before"], "->", trees[2]["goal_after"],
              "flags", trees[2]["skip_set"])
        out[name] = dict(partial=bool(partial), trees=trees)
    path = os.path.join(HERE, "rrt_revalidate.json")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(out[k], sort_keys=True)) for k in sorted(out)) + "\n}\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
