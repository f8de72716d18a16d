#!/usr/bin/env python3
"""Golden vectors for PRM over SO3StateSpace (oxhip_prm_config.space = OXHIP_SPACE_SO3, prm_so3.hip): an independent pure-Python
restatement of oxmpl's PRM (oxmpl/src/geometric/planners/prm.rs:96-154 construct, :161-187 check_motion, :227-307 solve with
its breadth-first search, :189-208 path) with the SO(3) operations of make_golden_so3.py (distance, interpolate,
sample_uniform, the cone checker, check_motion) and make_golden.py's ChaCha12 stream.  It is the CPU checker of the SO(3) PRM
tests; run it to (re)generate tests/golden/prm_so3_golden.json (well under a minute).

The reference samples for `timeout` seconds; the device path stops at max_milestones / max_samples, which this checker applies
where the reference reads its clock (before every sample_uniform call).  acos / sin are ox_acos / ox_sincos: PARITY UNPINNED
against a libm-built oxmpl, as for SO(3) RRT (DESIGN.md sections 14, 15).

    python tests/golden/make_golden_prm_so3.py
"""
import json
import os
import sys
from collections import deque

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (ChaCha12Rng, hexf)
from make_golden_so3 import (PI, Cones, check_motion, distance, normalise, quaternion_from_axis_angle,  # noqa: E402
                             sample_uniform, space_bounds)


def prm_construct(bounds, radius, fraction, cones, seed, stream, max_milestones, max_samples):
    """prm.rs:96-154 over SO(3): sample_uniform -> is_valid -> every earlier milestone i ascending:
    distance(q, m_i) < radius && check_motion(q -> m_i) -> edge both ways"""
    centre, max_angle = space_bounds(bounds)
    rng = mg.ChaCha12Rng(seed, stream)
    states, edges = [], []
    n_samples = 0
    while len(states) < max_milestones and n_samples < max_samples:
        q = sample_uniform(rng, centre, max_angle)            # so3_state_space.rs:201-231
        n_samples += 1
        if not cones.is_valid(q):                             # prm.rs:123
            continue
        mine = [i for i, m in enumerate(states) if distance(q, m) < radius and check_motion(cones, fraction, q, m)]
        new_idx = len(states)
        states.append(q)
        edges.append(mine)
        for i in mine:
            edges[i].append(new_idx)                          # prm.rs:143-145
    return dict(states=states, edges=edges, n_samples=n_samples, draws=rng.draws)


def prm_solve(radius, fraction, cones, rm, start, target, goal_r):
    """prm.rs:227-307; returns (status, start_connections, goal_indices, path) -- the BFS of make_golden_prm.prm_solve"""
    states, edges = rm["states"], rm["edges"]
    n = len(states)
    if n == 0:
        return "unsampled", [], [], []
    if not cones.is_valid(start):
        return "invalid_start", [], [], []
    sc = [i for i in range(n) if distance(start, states[i]) < radius and check_motion(cones, fraction, start, states[i])]
    gi = [i for i in range(n) if distance(states[i], target) <= goal_r]
    if not sc or not gi:
        return "no_solution", sc, gi, []
    goal_set = set(gi)
    queue = deque(sc)                     # prm.rs:271
    parent = {}
    visited = [False] * n
    for i in sc:                          # prm.rs:275-279 (second enqueue)
        queue.append(i)
        parent[i] = None
        visited[i] = True
    reached = None
    while queue:
        cur = queue.popleft()
        if cur in goal_set:
            reached = cur
            break
        for nb in edges[cur]:
            if not visited[nb]:
                visited[nb] = True
                parent[nb] = cur
                queue.append(nb)
    if reached is None:
        return "no_solution", sc, gi, []
    chain = []
    cur = reached
    while parent[cur] is not None:        # prm.rs:199-203
        chain.append(cur)
        cur = parent[cur]
    chain.append(cur)
    chain.reverse()
    return "solved", sc, gi, [list(start)] + [list(states[i]) for i in chain]


# ------------------------------------------------------------------------------------------------------------- scenes
def fixture_scene():
    """test_prm_finds_path_in_so3ss (oxmpl/tests/prm_so3ss_tests.rs): PRM::new(5.0, 0.5), unbounded space, one forbidden cone
    of 44.9 degrees about the identity, start / goal a quarter turn either way about y, goal radius 10 degrees"""
    return dict(bounds=None, radius=0.5, fraction=0.05, cones=[([0.0, 0.0, 0.0, 1.0], 44.9 * (PI / 180.0))],
                seed=11, stream=0, max_milestones=500, max_samples=10 ** 9,
                queries=[(quaternion_from_axis_angle([0.0, 1.0, 0.0], PI / 2.0), quaternion_from_axis_angle([0.0, 1.0, 0.0], -PI / 2.0),
                          10.0 * (PI / 180.0))])


def scenes():
    fx = fixture_scene()
    s, g, gr = fx["queries"][0]
    out = {"fixture": dict(fx, queries=[(s, g, gr),
                                         (g, s, gr),                                          # a second query (set_problem)
                                         ([0.0, 0.0, 0.0, 1.0], g, gr),                       # start inside the cone
                                         (normalise([0.3, 0.1, -0.2, 0.9]), normalise([-0.5, 0.5, 0.5, 0.5]), 0.2)])}
    c1 = normalise([0.1, 0.2, -0.3, 0.9])
    out["bounded"] = dict(bounds=(c1, 1.0), radius=0.3, fraction=0.05,
                          cones=[(normalise([-0.03, 0.13, -0.3, 0.78]), 0.25), (normalise([0.1, 0.3, -0.45, 0.8]), 0.15),
                                 (normalise([0.3, 0.1, -0.1, 0.9]), 0.2)],
                          seed=5, stream=3, max_milestones=400, max_samples=10 ** 9,
                          queries=[(normalise([0.3, -0.2, -0.1, 0.9]), normalise([-0.2, 0.45, -0.4, 0.75]), 0.2),
                                   (normalise([-0.2, 0.45, -0.4, 0.75]), normalise([0.3, -0.2, -0.1, 0.9]), 0.2)])
    out["wide_radius"] = dict(bounds=None, radius=2.0, fraction=0.05, cones=fx["cones"], seed=2, stream=7, max_milestones=60,
                              max_samples=10 ** 9, queries=[(s, g, gr)])
    out["tiny_radius"] = dict(bounds=None, radius=1e-3, fraction=0.05, cones=fx["cones"], seed=3, stream=1, max_milestones=300,
                              max_samples=10 ** 9, queries=[(s, g, gr)])
    cd = normalise([0.6, 0.2, 0.1, 0.5])   # (outside the cone: a valid centre)
    out["degenerate"] = dict(bounds=(cd, 1e-10), radius=0.5, fraction=0.05, cones=fx["cones"], seed=4, stream=0, max_milestones=24,
                             max_samples=10 ** 9, queries=[(cd, cd, 0.1)])
    out["sample_cap"] = dict(fx, seed=9, stream=4, max_milestones=10 ** 6, max_samples=150, queries=[(s, g, gr)])
    return out


def run_scene(sc):
    cones = Cones(sc["cones"])
    rm = prm_construct(sc["bounds"], sc["radius"], sc["fraction"], cones, sc["seed"], sc["stream"], sc["max_milestones"],
                       sc["max_samples"])
    queries = [prm_solve(sc["radius"], sc["fraction"], cones, rm, st, tg, gr) for st, tg, gr in sc["queries"]]
    return rm, queries


def scene_params(sc):
    hx = lambda row: [mg.hexf(v) for v in row]  # noqa: E731
    return dict(bounds=None if sc["bounds"] is None else [hx(sc["bounds"][0]), mg.hexf(sc["bounds"][1])],
                radius=mg.hexf(sc["radius"]), fraction=mg.hexf(sc["fraction"]), cones=[[hx(c), mg.hexf(r)] for c, r in sc["cones"]],
                seed=sc["seed"], stream=sc["stream"], max_milestones=sc["max_milestones"], max_samples=sc["max_samples"],
                queries=[[hx(st), hx(tg), mg.hexf(gr)] for st, tg, gr in sc["queries"]])


def record(rm, queries):
    return dict(n=len(rm["states"]), n_samples=rm["n_samples"], draws=rm["draws"],
                states=[[mg.hexf(v) for v in row] for row in rm["states"]], edges=[list(e) for e in rm["edges"]],
                queries=[dict(status=st, start_connections=sc, goal_indices=gi, path=[[mg.hexf(v) for v in row] for row in path])
                         for st, sc, gi, path in queries])


def main():
    out = {"_generator": "tests/golden/make_golden_prm_so3.py",
           "_parity": "UNPINNED: acos / sin are the build's ox_acos / ox_sincos; the reference cannot be built here"}
    for name, sc in scenes().items():
        rm, queries = run_scene(sc)
        out[name] = dict(params=scene_params(sc), run=record(rm, queries))
        print(name, "n", len(rm["states"]), "samples", rm["n_samples"], "draws", rm["draws"],
              "edge entries", sum(len(e) for e in rm["edges"]), [(q[0], len(q[1]), len(q[2]), len(q[3])) for q in queries])
    path = os.path.join(HERE, "prm_so3_golden.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("wrote", path)


if __name__ == "__main__":
    main()
