"""CPU: the definitions behind oxhip_prm_solve_batch_shortest, on the pure-Python checker
(tests/golden/make_golden_prm_shortest.py) and random graphs that hold what breaks a careless definition: zero weights (parent
cycles), weights lost in rounding (1e-20 beside 1.0: equal labels along an edge of positive weight) and exact ties.
(i)   the labels -- the least solution of c[v] = min(init[v], min_u fl(c[u] + w(u, v))) -- are the same from Dijkstra and from
      Bellman-Ford sweeps in several random orders: the fixed point does not depend on the order of relaxations;
(ii)  the tight levels reach exactly the finite labels, and every parent chain ends at a source after `hops` steps;
(iii) unit and zero weights give the same node lists, of the length the literal FIFO of prm.rs:270-301 finds."""
import os
import random
import sys
from collections import deque

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_prm_shortest as gsp  # noqa: E402

INF = gsp.INF
WEIGHTS = (0.0, 0.0, 1e-20, 1e-20, 1.0, 1.0, 0.5, 0.25, 0.1, 0.3)


def random_graph(rng):
    """-> (edges ascending, W symmetric, init, gi): an undirected graph, a few start connections, a few goal milestones"""
    n = rng.randint(2, 40)
    p = rng.choice((0.05, 0.1, 0.3, 1.0))
    w = {}
    for u in range(n):
        for v in range(u + 1, n):
            if rng.random() < p:
                w[(u, v)] = w[(v, u)] = rng.choice(WEIGHTS) if rng.random() < 0.8 else rng.random()
    edges = [[v for v in range(n) if (u, v) in w] for u in range(n)]
    W = [[w[(u, v)] for v in lst] for u, lst in enumerate(edges)]
    init = [INF] * n
    for m in rng.sample(range(n), rng.randint(1, min(n, 4))):
        init[m] = rng.choice(WEIGHTS) if rng.random() < 0.7 else rng.random()
    gi = sorted(rng.sample(range(n), rng.randint(1, min(n, 4))))
    return edges, W, init, gi


def literal_bfs_length(edges, sc, gi):
    """prm.rs:270-301: milestones on the path to the first goal milestone dequeued, or None"""
    queue, depth = deque(sc), {m: 1 for m in sc}
    while queue:
        cur = queue.popleft()
        if cur in gi:
            return depth[cur]
        for nb in edges[cur]:
            if nb not in depth:
                depth[nb] = depth[cur] + 1
                queue.append(nb)
    return None


@pytest.mark.parametrize("seed", range(6))
def test_labels_levels_and_chains_on_random_graphs(seed):
    rng = random.Random(1000 + seed)
    reached_by_zero_weight = lost_in_rounding = ties = 0
    for _ in range(50):
        edges, W, init, gi = random_graph(rng)
        n = len(edges)
        res = gsp.shortest_query(edges, W, init, gi)              # (asserts that levels reach exactly the finite labels)
        c, hops, parent = res["c"], res["hops"], res["parent"]
        for _ in range(3):                                        # (i)
            order = list(range(n))
            rng.shuffle(order)
            assert gsp.labels_bellman_ford(edges, W, init, order) == c
        for v in range(n):                                        # (ii)
            if c[v] == INF:
                assert hops[v] == gsp.UNSET and parent[v] == gsp.UNSET
                continue
            assert c[v] <= init[v]
            x, steps = v, 0
            while parent[x] != gsp.ROOT:
                u = parent[x]
                k = edges[u].index(x)
                assert c[u] + W[u][k] == c[x] and hops[u] == hops[x] - 1
                tight_up = [y for j, y in enumerate(edges[x]) if c[y] + W[x][j] == c[x] and hops[y] == hops[x] - 1]
                assert u == min(tight_up)                         # the lowest-index tight predecessor one level up
                reached_by_zero_weight += W[u][k] == 0.0
                lost_in_rounding += W[u][k] > 0.0 and c[u] == c[x]
                ties += len(tight_up) > 1
                x, steps = u, steps + 1
            assert steps == hops[v] and init[x] == c[x]           # the chain ends at a source after `hops` steps
        if res["status"] == "solved":
            g = res["goal"]
            assert (c[g], hops[g], g) == min((c[x], hops[x], x) for x in gi if c[x] < INF)
            assert len(res["nodes"]) == hops[g] + 1 and res["nodes"][-1] == g
            cost = init[res["nodes"][0]]
            for a, b in zip(res["nodes"], res["nodes"][1:]):
                cost = cost + W[a][edges[a].index(b)]
            assert cost == res["cost"]                            # the left-to-right sum is the label, bit for bit
        else:
            assert all(c[x] == INF for x in gi)
    assert reached_by_zero_weight and lost_in_rounding and ties   # the graphs hold what they are meant to hold


@pytest.mark.parametrize("seed", range(4))
def test_unit_and_zero_weights_give_the_fifo_length(seed):
    rng = random.Random(2000 + seed)
    solved = 0
    for _ in range(60):
        edges, _, init, gi = random_graph(rng)
        sc = [m for m in range(len(edges)) if init[m] < INF]
        res = {}
        for mode, w in ((gsp.UNIT, 1.0), (gsp.ZERO, 0.0)):
            W = [[w] * len(lst) for lst in edges]
            res[mode] = gsp.shortest_query(edges, W, [w if m in sc else INF for m in range(len(edges))], gi)
        assert res[gsp.UNIT]["status"] == res[gsp.ZERO]["status"] and res[gsp.UNIT]["nodes"] == res[gsp.ZERO]["nodes"]
        assert res[gsp.UNIT]["hops"] == res[gsp.ZERO]["hops"] and res[gsp.UNIT]["parent"] == res[gsp.ZERO]["parent"]
        want = literal_bfs_length(edges, sc, set(gi))
        assert (len(res[gsp.UNIT]["nodes"]) or None) == want
        solved += want is not None
    assert solved >= 20
