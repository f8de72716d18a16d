"""CPU: the scenes of tests/rrt_star_limits_shapes.py hold what tests/test_gpu_rrt_star_limits.py needs them to hold, and the two
restatements of RRTStar::solve -- the C oracle (oracle/rrt_oracle.c) and the instrumented numpy replay -- agree bit for bit on them:
states, parents after rewiring, costs, checksum; for the first time outside R^2 / R^3 and on tie-heavy input.  The GPU test compares
the device with the oracle bit for bit, so these conditions on the INPUT carry over to the device's run: a slab scene rewires, changes
parents and has neighbour motions refused by spheres beyond the 64th in every dimension; a reach scene has thousands of exact cost
ties, lists longer than 64 entries and a minimum shared between two 64-entry blocks; the large tree has parents beyond 2^15; the mixed
batch has problems of 2 nodes next to problems at the node cap, and
problems that end only at a bit-equal copy of their goal.  The counters are printed: the run's output is the record."""
import numpy as np
import pytest

import rrt_star_limits_shapes as shapes
from helpers import bits

DIMS = range(1, 9)
N_MIXED = len(shapes.MIXED_RADII)


def _assert_restatements_agree(res, o):
    assert (res["n"], res["iterations"], res["accepted"], res["goal_node"]) == (o.num_nodes, o.iterations, o.accepted, o.goal_node)
    assert res["checksum"] == o.checksum
    states, parents = o.tree()
    assert np.array_equal(bits(states), bits(res["states"]))
    assert [int(v) for v in parents] == res["parents"]
    assert np.array_equal(bits(o.costs()), bits(np.array(res["cost"])))


@pytest.mark.parametrize("dim", DIMS)
def test_slab_scene(dim):
    P = shapes.slab_scene(dim)
    res = shapes.slab_replay(dim)
    k = res["counters"]
    print("slab R^%d" % dim, "spheres", len(P["spheres"]), "nodes", res["n"], "iterations", res["iterations"], k)
    assert res["n"] == P["max_nodes"] == 600
    assert shapes.BLOCK < len(P["spheres"]) <= 100 and len(P["boxes"]) == 1          # a second sphere chunk, and a box with them
    _assert_restatements_agree(res, shapes.slab_oracle(dim, shapes.PIDS[0]))
    if dim >= 2:
        assert k["rewires"] >= 300 and k["changed_parents"] >= 200 and k["rejected"] >= 200 and k["late_only"] >= 50
    for pid in shapes.PIDS[1:]:
        assert shapes.slab_oracle(dim, pid).num_nodes == 600


@pytest.mark.parametrize("variant", shapes.REACH_VARIANTS)
@pytest.mark.parametrize("dim", DIMS)
def test_reach_scene(dim, variant):
    P = shapes.reach_scene(dim, variant)
    res = shapes.reach_replay(dim, variant)
    k = res["counters"]
    print("reach R^%d %s" % (dim, variant), "nodes", res["n"], "iterations", res["iterations"], k)
    assert res["n"] == P["max_nodes"] == 300
    _assert_restatements_agree(res, shapes.reach_oracle(dim, variant, shapes.PIDS[0]))
    copies = int((bits(res["states"]) == bits(np.array(P["goal_c"]))).all(axis=1).sum())
    # bit-equal copies of the goal centre (on the line the box shuts the goal off: there the ties are those of collinear nodes)
    assert copies >= 100 or (dim == 1 and variant == "box" and copies == 0)
    assert k["parent_ties"] >= 1000 and k["rewire_ties"] >= 1000 and k["long_lists"] >= 20
    assert k["shared_minima"] >= 1 and k["cross_block_minima"] >= 1
    for pid in shapes.PIDS[1:]:
        assert shapes.reach_oracle(dim, variant, pid).num_nodes == 300


def test_replay_check_motion_is_the_checkers():
    """the replay evaluates a motion's states as rows; make_golden.check_motion one by one: same verdicts on the R^3 slab's own
    neighbour motions, both kinds among them"""
    P = shapes.slab_scene(3)
    field = shapes.mg.Field(3, P["spheres"], P["boxes"])
    st = shapes.slab_replay(3)["states"]
    seen = set()
    for i in range(1, 600, 3):
        for j in (0, i // 2, i - 1):
            a, b = [float(v) for v in st[i]], [float(v) for v in st[j]]
            want = shapes.mg.check_motion(field, P["bounds"], P["fraction"], a, b)
            assert shapes.check_motion(field, P["bounds"], P["fraction"], a, b) == want
            seen.add(want)
    assert seen == {True, False}


def test_large_tree_names_nodes_beyond_two_to_the_fifteenth():
    o = shapes.large_oracle()
    _, parents = o.tree()
    far = int((parents >= shapes.HALF_U16).sum())
    print("large tree: nodes", o.num_nodes, "iterations", o.iterations, "parents of 2^15 or more", far, "goal node", o.goal_node)
    assert o.num_nodes == 33000 and far >= 100


@pytest.mark.parametrize("dim", [3, 5])
def test_mixed_batch_two_calls(dim):
    P = shapes.mixed_scene(dim, "two_calls")
    first, second = shapes.MIXED_RUNS["two_calls"][1]
    assert P["max_nodes"] == 500 and P["search_radius"] == shapes.INF and first == 60
    after_first = [shapes.mixed_geometry(dim, "two_calls", p, first) for p in range(N_MIXED)]
    at_end = [shapes.mixed_geometry(dim, "two_calls", p, first + second) for p in range(N_MIXED)]
    print("mixed R^%d two calls: (nodes, goal node) after 60" % dim, after_first, "at the end", at_end)
    for p, radius in enumerate(shapes.MIXED_RADII):
        if radius == 100.0:
            assert after_first[p] == at_end[p] == (2, 1)                             # ends at its first inserted node
        if radius == 0.0:                                                            # ends, but only at a bit-equal copy of its goal
            n, goal_node = at_end[p]
            assert goal_node == n - 1 and 2 < n < 500
            states, _ = shapes.mixed_oracle(dim, "two_calls", p, first + second).tree()
            assert len(states) == n and np.array_equal(bits(states[-1]), bits(np.array(P["goal_c"])))
        if radius < 0.0:
            assert at_end[p] == (500, -1)                                            # never ends: the node cap
            pending = shapes.entries_between(after_first[p][0], at_end[p][0])
            print("  problem", p, "brings", pending, "entries to the second call")
            assert pending >= shapes.EIGHT_SEGMENTS_FROM
            rounds = shapes.wiring_rounds(after_first[p][0], at_end[p][0], 500)
            print("  in rounds of", rounds)
            assert len(rounds) >= 2 and max(rounds) < shapes.EIGHT_SEGMENTS_FROM       # (one_call below is where a round reaches it)
    assert len({n for n, _ in at_end}) >= 4                                          # problems of one batch that differ
    for p in (0, 4, 9):                                                              # the oracle's counts are the geometry's
        o = shapes.mixed_oracle(dim, "two_calls", p, first + second)
        assert (o.num_nodes, o.goal_node) == at_end[p]


@pytest.mark.parametrize("dim", [3, 5])
def test_mixed_batch_one_call_reaches_eight_segments(dim):
    """one entry next to a round of more than 65,536: the pool segment at 1,100 nodes (capacity 2,048) holds 131,072 entries"""
    P = shapes.mixed_scene(dim, "one_call")
    at_end = [shapes.mixed_geometry(dim, "one_call", p, shapes.BUDGET) for p in range(N_MIXED)]
    print("mixed R^%d one call: (nodes, goal node)" % dim, at_end)
    assert at_end[0] == at_end[1] == (2, 1) and shapes.entries_between(1, 2) == 1
    assert at_end[8] == at_end[9] == (P["max_nodes"], -1)
    rounds = shapes.wiring_rounds(1, P["max_nodes"], P["max_nodes"])
    print("  rounds of a capped problem:", rounds, "of", shapes.entries_between(1, P["max_nodes"]), "entries")
    assert sum(rounds) == shapes.entries_between(1, P["max_nodes"])
    assert rounds[0] >= shapes.EIGHT_SEGMENTS_FROM and len(rounds) >= 2              # eight segments, and further rounds
