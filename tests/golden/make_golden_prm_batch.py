#!/usr/bin/env python3
"""Generates tests/golden/prm_batch_golden.json: 32 seeded queries on each of three roadmaps of the existing generators -- the
`wall` and `r6` scenes of make_golden_prm.py and the SO(3) `fixture` scene of make_golden_prm_so3.py -- answered one by one by
those generators' prm_solve, i.e. by the literal FIFO of prm.rs:270-301.  This is what a batch (oxhip_prm_solve_batch) has to
return query by query: status, the sizes of both query sets, the goal milestone reached and the path's rows, bit for bit.

The roadmaps themselves are pinned by prm_golden.json / prm_so3_golden.json; this file records the queries only.

    python tests/golden/make_golden_prm_batch.py      (about a minute)
"""
import json
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import make_golden_prm as gp  # noqa: E402
import make_golden_prm_so3 as gs  # noqa: E402
from make_golden_so3 import Cones, normalise  # noqa: E402

N_QUERIES = 32
SEED = 20261016


def rn_queries(scene, dim, r_lo, r_hi):
    """starts, then goal centres, uniform in [0, 10)^dim; then goal radii uniform in [r_lo, r_hi)"""
    rng = np.random.default_rng([SEED, {"wall": 0, "r6": 1}[scene]])
    starts = rng.uniform(0.0, 10.0, size=(N_QUERIES, dim))
    goals = rng.uniform(0.0, 10.0, size=(N_QUERIES, dim))
    radii = rng.uniform(r_lo, r_hi, size=N_QUERIES)
    return [([float(v) for v in s], [float(v) for v in g], float(r)) for s, g, r in zip(starts, goals, radii)]


def so3_queries():
    """normalised Gaussian quaternions: starts, then targets; then goal radii uniform in [0.2, 0.6)"""
    rng = np.random.default_rng([SEED, 2])
    starts = rng.standard_normal(size=(N_QUERIES, 4))
    goals = rng.standard_normal(size=(N_QUERIES, 4))
    radii = rng.uniform(0.2, 0.6, size=N_QUERIES)
    return [(normalise([float(v) for v in s]), normalise([float(v) for v in g]), float(r)) for s, g, r in zip(starts, goals, radii)]


def rn_scene(scene):
    """the roadmap of make_golden_prm.main()'s scene of that name, rebuilt from the parameters prm_golden.json records"""
    with open(os.path.join(HERE, "prm_golden.json")) as f:
        P = json.load(f)[scene]["params"]
    unhex = lambda v: struct.unpack("<d", struct.pack("<Q", int(v, 16)))[0] if isinstance(v, str) else v  # noqa: E731
    spheres = [([unhex(v) for v in c], unhex(r)) for c, r in P["spheres"]]
    field = gp.Field(P["dim"], spheres, P["boxes"])
    bounds = [tuple(b) for b in P["bounds"]]
    rm = gp.prm_construct(P["dim"], bounds, P["radius"], P["fraction"], field, P["seed"], P["stream"], P["max_milestones"], P["max_samples"])
    return P, bounds, field, rm


def entry(start, goal_c, goal_r, status, sc, gi, path, states):
    goal_node = -1
    if status == "solved":
        last = [float(v) for v in path[-1]]
        goal_node = next(i for i in gi if [float(v) for v in states[i]] == last)   # milestones are distinct samples
    return dict(start=[mg.hexf(v) for v in start], goal_c=[mg.hexf(v) for v in goal_c], goal_r=mg.hexf(goal_r), status=status,
                n_start=len(sc), n_goal=len(gi), goal_node=goal_node, path=[[mg.hexf(v) for v in row] for row in path])


def main():
    out = {"_generator": "tests/golden/make_golden_prm_batch.py",
           "_roadmaps": "wall, r6: prm_golden.json params; fixture: make_golden_prm_so3.scenes()['fixture']"}
    for scene, (r_lo, r_hi) in (("wall", (0.3, 0.8)), ("r6", (2.0, 3.5))):
        P, bounds, field, rm = rn_scene(scene)
        qs = []
        for start, goal_c, goal_r in rn_queries(scene, P["dim"], r_lo, r_hi):
            status, sc, gi, path = gp.prm_solve(P["dim"], bounds, P["radius"], P["fraction"], field, rm, start, goal_c, goal_r)
            qs.append(entry(start, goal_c, goal_r, status, sc, gi, path, rm["states"]))
        out[scene] = dict(space="real_vector", n=len(rm["edges"]), queries=qs)
    sc3 = gs.scenes()["fixture"]
    cones = Cones(sc3["cones"])
    rm = gs.prm_construct(sc3["bounds"], sc3["radius"], sc3["fraction"], cones, sc3["seed"], sc3["stream"], sc3["max_milestones"],
                          sc3["max_samples"])
    qs = []
    for start, target, goal_r in so3_queries():
        status, sc, gi, path = gs.prm_solve(sc3["radius"], sc3["fraction"], cones, rm, start, target, goal_r)
        qs.append(entry(start, target, goal_r, status, sc, gi, path, rm["states"]))
    out["fixture"] = dict(space="so3", n=len(rm["states"]), queries=qs)
    for name in ("wall", "r6", "fixture"):
        qs = out[name]["queries"]
        print(name, "n", out[name]["n"], {s: sum(q["status"] == s for q in qs) for s in ("solved", "no_solution", "invalid_start")},
              "longest path", max(len(q["path"]) for q in qs))
    path = os.path.join(HERE, "prm_batch_golden.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
