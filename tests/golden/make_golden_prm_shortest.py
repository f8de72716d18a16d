#!/usr/bin/env python3
"""Generates tests/golden/prm_shortest_golden.json, and is the pure-Python checker of oxhip_prm_solve_batch_shortest (DESIGN.md
section 19): the 32 queries of each scene of make_golden_prm_batch.py (`wall`, `r6`, the SO(3) `fixture`), answered with shortest
paths on the same roadmaps, with the same query sets (the generators' prm_solve) and the same distance functions.

    labels   c = the least solution of c[v] = min(init[v], min over neighbours u of fl(c[u] + w(u, v))): Dijkstra
    tight    u -> v iff fl(c[u] + w(u, v)) == c[v]; sources = the start connections m with c[m] == init[m]
    hops     breadth-first depth from the sources over tight edges; parent = lowest-index tight predecessor one level up
    answer   the goal milestone of least (c, hops, index); nodes = its parent chain from a source

Per query the file records the status, the cost (hex) and the node list for distance weights, and the node list for unit weights.

    python tests/golden/make_golden_prm_shortest.py      (about ten seconds)
"""
import heapq
import json
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

INF = float("inf")
ROOT = 0x7FFFFFFF          # parent of a source
UNSET = 0xFFFFFFFF         # hops / parent of a milestone no finite label reaches
DISTANCE, UNIT, ZERO = 0, 1, 2
SOLVED_COUNTS = {"wall": 31, "r6": 11, "fixture": 23}
DIFFER_FROM_BFS = {"wall": 29, "r6": 6, "fixture": 23}


def hexf(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", v))[0]


def unhex(s):
    return struct.unpack("<d", struct.pack("<Q", int(s, 16)))[0]


def edge_weights(edges, states, dist, mode=DISTANCE):
    """W[u][k] = w(u, edges[u][k])"""
    if mode != DISTANCE:
        return [[1.0 if mode == UNIT else 0.0] * len(lst) for lst in edges]
    rows = [[float(x) for x in s] for s in states]
    return [[dist(rows[u], rows[v]) for v in lst] for u, lst in enumerate(edges)]


def init_labels(n, sc, start, states, dist, mode=DISTANCE):
    init = [INF] * n
    for m in sc:
        init[m] = dist(list(start), [float(x) for x in states[m]]) if mode == DISTANCE else (1.0 if mode == UNIT else 0.0)
    return init


def labels_dijkstra(edges, W, init):
    c = list(init)
    heap = [(v, i) for i, v in enumerate(c) if v < INF]
    heapq.heapify(heap)
    done = [False] * len(c)
    while heap:
        cu, u = heapq.heappop(heap)
        if done[u] or cu != c[u]:
            continue
        done[u] = True
        for k, v in enumerate(edges[u]):
            nv = cu + W[u][k]                   # one rounded binary64 add
            if nv < c[v]:
                c[v] = nv
                heapq.heappush(heap, (nv, v))
    return c


def labels_bellman_ford(edges, W, init, order):
    """sweeps over the nodes in the given order until nothing changes: any order reaches the same least fixed point"""
    c = list(init)
    changed = True
    sweeps = 0
    while changed:
        changed = False
        sweeps += 1
        assert sweeps <= len(c) + 1
        for u in order:
            if c[u] == INF:
                continue
            for k, v in enumerate(edges[u]):
                nv = c[u] + W[u][k]
                if nv < c[v]:
                    c[v] = nv
                    changed = True
    return c


def tight_levels(edges, W, c, init):
    n = len(c)
    hops, parent = [UNSET] * n, [UNSET] * n
    level = [m for m in range(n) if init[m] < INF and init[m] == c[m]]
    for m in level:
        hops[m], parent[m] = 0, ROOT
    depth = 0
    while level:
        nxt = []
        for u in level:
            for k, v in enumerate(edges[u]):
                nv = c[u] + W[u][k]
                if nv == c[v] and nv < INF and hops[v] == UNSET:
                    if parent[v] == UNSET:
                        nxt.append(v)
                    parent[v] = min(parent[v], u)
        for v in nxt:
            hops[v] = depth + 1
        level = nxt
        depth += 1
    return hops, parent


def shortest_query(edges, W, init, gi):
    """-> dict(status, cost, goal, nodes, c, hops, parent) for a query with a valid start whose sets are (init's support, gi)"""
    c = labels_dijkstra(edges, W, init)
    hops, parent = tight_levels(edges, W, c, init)
    for v in range(len(c)):
        assert (c[v] < INF) == (hops[v] != UNSET), v          # tight levels reach exactly the finite labels
    best = min(((c[g], hops[g], g) for g in gi if c[g] < INF), default=None)
    out = dict(status="no_solution", cost=INF, goal=-1, nodes=[], c=c, hops=hops, parent=parent)
    if best is None:
        return out
    chain, v = [], best[2]
    while v != ROOT:
        chain.append(v)
        assert hops[v] + len(chain) - 1 == best[1]
        v = parent[v]
    assert len(chain) == best[1] + 1                          # the chain has hops + 1 milestones
    chain.reverse()
    out.update(status="solved", cost=best[0], goal=best[2], nodes=chain)
    return out


def path_cost(start, nodes, states, dist):
    """the left-to-right sum of the path's edge distances"""
    rows = [list(start)] + [[float(x) for x in states[i]] for i in nodes]
    cost = dist(rows[0], rows[1])
    for a, b in zip(rows[1:], rows[2:]):
        cost = cost + dist(a, b)
    return cost


def answer_scene(edges, states, dist, queries):
    """queries: list of (status, sc, gi, start) as the generators' prm_solve returns them -> the records of the golden file"""
    n = len(edges)
    W = {mode: edge_weights(edges, states, dist, mode) for mode in (DISTANCE, UNIT)}
    out = []
    for status, sc, gi, start in queries:
        rec = dict(status=status, cost=hexf(INF), nodes=[], nodes_unit=[])
        if status != "invalid_start" and sc and gi:
            res = {mode: shortest_query(edges, W[mode], init_labels(n, sc, start, states, dist, mode), gi) for mode in (DISTANCE, UNIT)}
            assert res[DISTANCE]["status"] == res[UNIT]["status"] == status
            if status == "solved":
                assert hexf(path_cost(start, res[DISTANCE]["nodes"], states, dist)) == hexf(res[DISTANCE]["cost"])
                rec.update(cost=hexf(res[DISTANCE]["cost"]), nodes=res[DISTANCE]["nodes"], nodes_unit=res[UNIT]["nodes"])
        out.append(rec)
    return out


def check_against_bfs(recs, bfs, states, dist):
    """recs: a scene's records here; bfs: the same queries in prm_batch_golden.json.  Same statuses; every recorded path's
    left-to-right cost is its label bit for bit and no more than the BFS path's.  -> (solved, paths that differ from BFS's, largest
    BFS cost / shortest cost)"""
    assert [r["status"] for r in recs] == [q["status"] for q in bfs]
    solved = differ = 0
    ratio = 1.0
    for r, q in zip(recs, bfs):
        if r["status"] != "solved":
            assert r["nodes"] == [] and r["nodes_unit"] == [] and r["cost"] == hexf(INF)
            continue
        solved += 1
        start = [unhex(v) for v in q["start"]]
        rows = [[hexf(float(x)) for x in states[i]] for i in r["nodes"]]
        cost = path_cost(start, r["nodes"], states, dist)
        assert hexf(cost) == r["cost"]
        bfs_rows = [[unhex(v) for v in row] for row in q["path"]]
        bfs_cost = dist(bfs_rows[0], bfs_rows[1])
        for a, b in zip(bfs_rows[1:], bfs_rows[2:]):
            bfs_cost = bfs_cost + dist(a, b)
        assert cost <= bfs_cost
        ratio = max(ratio, bfs_cost / cost)
        differ += rows != q["path"][1:]
        assert len(r["nodes_unit"]) == len(q["path"]) - 1     # unit weights: the fewest hops, BFS's count
    return solved, differ, ratio


def build_scenes():
    """-> (the golden file's content, {scene: (states, distance function)})"""
    import make_golden as mg
    import make_golden_prm as gp
    import make_golden_prm_batch as gb
    import make_golden_prm_so3 as gs
    from make_golden_so3 import Cones, distance as so3_distance

    out = {"_generator": "tests/golden/make_golden_prm_shortest.py",
           "_queries": "query k of a scene is query k of that scene in prm_batch_golden.json"}
    kept = {}
    for scene, (r_lo, r_hi) in (("wall", (0.3, 0.8)), ("r6", (2.0, 3.5))):
        P, bounds, field, rm = gb.rn_scene(scene)
        qs = []
        for start, goal_c, goal_r in gb.rn_queries(scene, P["dim"], r_lo, r_hi):
            status, sc, gi, _ = gp.prm_solve(P["dim"], bounds, P["radius"], P["fraction"], field, rm, start, goal_c, goal_r)
            qs.append((status, sc, gi, start))
        out[scene] = dict(space="real_vector", n=len(rm["edges"]), queries=answer_scene(rm["edges"], rm["states"], mg.distance, qs))
        kept[scene] = (rm["states"], mg.distance)
    sc3 = gs.scenes()["fixture"]
    cones = Cones(sc3["cones"])
    rm = gs.prm_construct(sc3["bounds"], sc3["radius"], sc3["fraction"], cones, sc3["seed"], sc3["stream"], sc3["max_milestones"],
                          sc3["max_samples"])
    qs = []
    for start, target, goal_r in gb.so3_queries():
        status, sc, gi, _ = gs.prm_solve(sc3["radius"], sc3["fraction"], cones, rm, start, target, goal_r)
        qs.append((status, sc, gi, start))
    out["fixture"] = dict(space="so3", n=len(rm["states"]), queries=answer_scene(rm["edges"], rm["states"], so3_distance, qs))
    kept["fixture"] = (rm["states"], so3_distance)
    return out, kept


def main():
    out, kept = build_scenes()
    with open(os.path.join(HERE, "prm_batch_golden.json")) as f:
        batch = json.load(f)
    for name in ("wall", "r6", "fixture"):
        solved, differ, ratio = check_against_bfs(out[name]["queries"], batch[name]["queries"], kept[name][0], kept[name][1])
        print(name, "n", out[name]["n"], "solved", solved, "differ from BFS", differ, "BFS cost / shortest cost up to %.3f" % ratio)
        assert solved == SOLVED_COUNTS[name] and differ == DIFFER_FROM_BFS[name], (name, solved, differ)
    path = os.path.join(HERE, "prm_shortest_golden.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
