"""The argument prm_batch.hip's search kernel rests on, independent of the kernel: the reference's FIFO (prm.rs:270-301) --
the queue starts as the start connections in ascending order, enqueued twice; a node's parent is whoever dequeued first among
its neighbours; the answer is the first dequeued goal milestone -- equals a level-by-level evaluation in which
  * level 0 is the start connections, ascending, and a node's rank is its position in its level,
  * a level that holds goal milestones answers with the one of lowest rank,
  * otherwise every unvisited neighbour of the level takes as parent the level's node of MINIMUM RANK adjacent to it, and the
    next level is those neighbours ordered by (parent's rank, position in the parent's ascending edge list).
The literal queue is tests/golden/make_golden_prm_so3.prm_solve itself, fed graphs through stand-ins for its geometry."""
import os
import random
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_prm_so3 as gs  # noqa: E402


def level_search(edges, sources, goals):
    """(chain of milestones from a start connection to the goal milestone reached) or None -- what the kernel computes:
    claims by minimum rank (the order in which claims arrive is shuffled on purpose), then a count per parent and a prefix sum"""
    n = len(edges)
    unvisited, goal = object(), set(goals)
    parent = [unvisited] * n
    level = sorted(sources)
    for s in level:
        parent[s] = None
    rnd = random.Random(len(edges) * 7919 + len(sources))
    while level:
        hits = [r for r, u in enumerate(level) if u in goal]
        if hits:
            chain, cur = [], level[min(hits)]
            while cur is not None:
                chain.append(cur)
                cur = parent[cur]
            return chain[::-1]
        claim = {}
        arrivals = [(r, v) for r, u in enumerate(level) for v in edges[u] if parent[v] is unvisited]
        rnd.shuffle(arrivals)                                   # atomicMin: order of arrival is irrelevant
        for r, v in arrivals:
            claim[v] = min(claim.get(v, r), r)
        counts = [sum(1 for v in edges[u] if parent[v] is unvisited and claim[v] == r) for r, u in enumerate(level)]
        offsets = [sum(counts[:r]) for r in range(len(level))]  # exclusive prefix sum
        nxt = [None] * sum(counts)
        for r, u in enumerate(level):
            k = offsets[r]
            for v in edges[u]:                                  # as they stand in the parent's list
                if parent[v] is unvisited and claim[v] == r:
                    nxt[k] = v
                    k += 1
        for v in nxt:
            parent[v] = level[claim[v]]
        level = nxt
    return None


def literal_queue(monkeypatch, edges, sources, goals):
    """make_golden_prm_so3.prm_solve on the graph: states are the node numbers, the start is -1, the target -2"""
    src, gl = set(sources), set(goals)

    def distance(a, b):
        if a == -1:
            return 0.0 if b in src else 1.0
        return 0.0 if (b == -2 and a in gl) else 1.0

    class Free:
        def is_valid(self, q):
            return True

    monkeypatch.setattr(gs, "distance", distance)
    monkeypatch.setattr(gs, "check_motion", lambda cones, fraction, a, b: True)
    rm = dict(states=list(range(len(edges))), edges=edges)
    # SO(3) states are lists; here rows are ints, so the path is rebuilt from the chain's length instead of list(states[i])
    monkeypatch.setattr(gs, "list", lambda x: x, raising=False)
    status, sc, gi, path = gs.prm_solve(0.5, 0.05, Free(), rm, -1, -2, 0.5)
    assert sc == sorted(src) and gi == sorted(gl)
    return (path[1:] if status == "solved" else None), status


def random_graph(rng, n, density):
    edges = [[] for _ in range(n)]
    for j in range(n):
        for i in range(j):
            if rng.random() < density:
                edges[j].append(i)
                edges[i].append(j)
    return [sorted(e) for e in edges]       # ascending, duplicate-free: the CSR of the key sort


def check(monkeypatch, edges, sources, goals):
    want, status = literal_queue(monkeypatch, edges, sources, goals)
    got = level_search(edges, sources, goals)
    assert got == want, (edges, sources, goals)
    return status


def test_level_order_equals_the_literal_queue_on_random_graphs(monkeypatch):
    rng = random.Random(20261016)
    solved = 0
    for _ in range(3000):
        n = rng.randint(1, 60)
        edges = random_graph(rng, n, rng.choice([0.02, 0.05, 0.1, 0.2, 0.4, 0.9]))
        sources = rng.sample(range(n), min(n, rng.randint(1, 6)))
        goals = rng.sample(range(n), min(n, rng.randint(1, 6)))
        solved += check(monkeypatch, edges, sources, goals) == "solved"
    assert 1500 < solved < 3000              # both outcomes are well represented


def test_a_source_that_is_itself_a_goal(monkeypatch):
    rng = random.Random(1)
    for _ in range(200):
        n = rng.randint(2, 40)
        edges = random_graph(rng, n, 0.2)
        sources = rng.sample(range(n), min(n, 4))
        goals = [sources[-1]] + rng.sample(range(n), 2)      # not the lowest source: the lowest-ranked goal of level 0 wins
        want, status = literal_queue(monkeypatch, edges, sources, goals)
        assert status == "solved" and len(want) == 1 and want[0] == min(set(sources) & set(goals))
        assert level_search(edges, sources, goals) == want


def test_unreachable_goals(monkeypatch):
    rng = random.Random(2)
    for _ in range(200):
        a, b = rng.randint(1, 25), rng.randint(1, 25)
        left, right = random_graph(rng, a, 0.3), random_graph(rng, b, 0.3)
        edges = left + [[v + a for v in e] for e in right]   # two components
        sources = rng.sample(range(a), min(a, 3))
        goals = [a + g for g in rng.sample(range(b), min(b, 3))]
        assert check(monkeypatch, edges, sources, goals) == "no_solution"


@pytest.mark.parametrize("n", [2, 3, 17, 64])
def test_complete_graphs(monkeypatch, n):
    rng = random.Random(n)
    edges = [[v for v in range(n) if v != u] for u in range(n)]
    for _ in range(50):
        sources = rng.sample(range(n), rng.randint(1, min(n, 5)))
        goals = rng.sample(range(n), rng.randint(1, min(n, 5)))
        assert check(monkeypatch, edges, sources, goals) == "solved"
        got = level_search(edges, sources, goals)
        if not set(sources) & set(goals):                    # every node hangs off the lowest source; the lowest goal is dequeued first
            assert got == [min(sources), min(goals)]
