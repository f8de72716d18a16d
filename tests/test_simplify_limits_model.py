"""CPU: the planted scenes of tests/simplify_limits_shapes.py hold what their docstrings claim and what tests/test_gpu_simplify_limits.py
relies on -- counted with the CPU oracle's check_motion / distance and the DP of tests/simplify_helpers.py -- the planted trees give the
paths back, and tests/golden/simplify_limits.json is what its generator writes today.  The oracle's verdicts are computed once, by the
generator's cache, and shared."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_simplify_limits as gen  # noqa: E402
import make_golden_so3 as so3  # noqa: E402

import rrt_revalidate_helpers as rh  # noqa: E402
import simplify_helpers as sh  # noqa: E402
import simplify_limits_shapes as shapes  # noqa: E402

SCENES = shapes.scenes()
LANES = shapes.LANES


def census(name, p, span):
    """the DP of shortcut_dp once more, counting: steps whose minimum two valid candidates share exactly (ties), tie steps whose winner
    is not the window's first index, steps where two tying candidates lie a multiple of 64 apart (one lane of path_dp_kernel holds both),
    steps whose parent lies more than 64 below; and both verdict counts"""
    L, valid, dist = gen.analysis(name, p)
    S = sh.span_of(L, span)
    cost, par = [0.0] * L, [0] * L
    out = dict(L=L, S=S, ties=0, not_first=0, same_lane=0, far=0)
    for j in range(1, L):
        base = max(0, j - S)
        cand = [(cost[i] + dist(i, j), i) for i in range(base, j) if j - i == 1 or valid[(i, j)]]
        best = min(c for c, _ in cand)
        at = [i for c, i in cand if c == best]
        cost[j], par[j] = best, at[0]
        out["ties"] += len(at) > 1
        out["not_first"] += len(at) > 1 and at[0] != base
        out["same_lane"] += any((b - a) % LANES == 0 for k, a in enumerate(at) for b in at[k + 1:])
        out["far"] += j - at[0] > LANES
    n_valid = sum(v for (i, j), v in valid.items() if j - i <= S)
    out["valid"], out["invalid"] = n_valid, sh.expected_checks(L, span) - n_valid
    idx = [L - 1]
    while idx[-1]:
        idx.append(par[idx[-1]])
    out["idx"] = idx[::-1]
    assert out["idx"] == gen.result(name, p, span)[0]
    return out


def test_corner_r2_holds_the_figures_of_its_docstring():
    c = census("corner_r2", 0, 0)
    print("corner_r2 full span:", c)
    assert c["idx"] == [0, 98, 100, 199]
    assert (c["ties"], c["not_first"], c["same_lane"], c["far"]) == (196, 98, 70, 70)
    assert (c["valid"], c["invalid"]) == (9802, 9899)
    c70 = census("corner_r2", 0, 70)
    print("corner_r2 span 70:", c70)
    assert c70["idx"] == [0, 28, 98, 100, 129, 199] and c70["ties"] >= 32


def test_line_free_r2_every_pair_valid_every_step_ties():
    for p, L in enumerate(shapes.LINE_LENGTHS):
        for span in shapes.spans_for(L):
            c = census("line_free_r2", p, span)
            print("line_free_r2 L", L, "span", span, c)
            assert c["invalid"] == 0 and c["ties"] == L - 2 and c["not_first"] == 0
            S = c["S"]
            want = list(range((L - 1) % S, L, S))
            assert c["idx"] == ([0] + want if want[0] else want)          # par[j] = max(0, j - S)
            wide = L - 1 - LANES if S > LANES else 0                       # steps whose window holds more than 64 candidates
            assert c["same_lane"] == c["far"] == wide and (wide > 0 or S <= LANES)


def test_arc_r2_both_verdicts_and_far_parents():
    for p, L in enumerate(shapes.ARC_LENGTHS):
        c = census("arc_r2", p, 0)
        print("arc_r2 L", L, c)
        assert c["valid"] >= 1000 and c["invalid"] >= 1000 or L == 66
        assert c["valid"] >= 100 and c["invalid"] >= 100
        if L >= 200:
            assert c["far"] >= 32
    c = census("arc_r2", shapes.ARC_LENGTHS.index(257), 65)
    assert c["far"] >= 1


def test_word_edges_slot_residues():
    res = shapes.word_residues()
    table = {r: sorted(k for k, v in res.items() if v == r and shapes.slot_count(*k)) for r in (0, LANES - 1, 1)}
    print("word_edges slots mod 64 -> (L, span):", table)
    assert table[0] == sorted(shapes.WORD_ON) and table[LANES - 1] == sorted(shapes.WORD_SHORT) and table[1] == sorted(shapes.WORD_PAST)
    scene = shapes.word_edges()
    assert tuple(shapes.length(q) for q in scene["problems"]) == shapes.WORD_LENGTHS
    seen = set()
    for p, L in enumerate(shapes.WORD_LENGTHS):
        if L >= 3:
            seen.update(gen.analysis("word_edges", p)[1].values())
    assert seen == {True, False}


def test_mixed_batch_rounds_have_equal_neighbours_at_start_middle_and_end():
    scene = shapes.mixed_batch()
    lengths = tuple(shapes.length(q) for q in scene["problems"])
    assert lengths == shapes.MIXED_LENGTHS
    where = set()
    for chunk in shapes.MIXED_CHUNKS:
        rounds = shapes.round_word_offsets(lengths, 0, chunk)
        assert len(rounds) == -(-len(lengths) // (chunk or len(lengths)))
        for woff in rounds:
            n = len(woff) - 1
            eq = [k for k in range(n) if woff[k] == woff[k + 1]]
            if n > 1 and woff[-1] > 0:   # a round with pairs and with a problem that has none
                where.update("start" if k == 0 else "end" if k == n - 1 else "middle" for k in eq)
        print("mixed_batch chunk", chunk, rounds)
    assert where == {"start", "middle", "end"}


@pytest.mark.parametrize("D", shapes.DIMS)
def test_dims_scene_holds_every_case_of_the_checker(D):
    name = "dims_r%d" % D
    scene = shapes.dims(D)
    problem = scene["problems"][0]
    path = problem["path"]
    L, valid, dist = gen.analysis(name, 0)
    c = census(name, 0, 0)
    n_s, n_b = len(scene["spheres"][1]), len(scene["boxes"][0])
    assert (L, n_s, n_b) == (70, 72, 3) and c["S"] == 69
    # which obstacle alone decides an invalid pair: the pair is valid without it
    inside = [(i, j) for (i, j), v in valid.items() if not v and i < shapes.DIMS_FAR[0] and j < shapes.DIMS_FAR[0]]
    sole = {}
    for k in list(range(LANES, n_s)) + [n_s + shapes.DIMS_BOX_C]:
        o = gen.rn_oracle(scene, problem, without=k)
        sole[k] = [ij for ij in inside if o.check_motion(path[ij[0]], path[ij[1]])]
    by_late_sphere = sum(len(sole[k]) for k in range(LANES, n_s))
    by_box = len(sole[n_s + shapes.DIMS_BOX_C])
    # the far nodes: 1000 to 10000 widths out, one in the last axis only; chords among them and to the arc, both verdicts
    W = shapes.DIMS_WIDTH
    out = [float(np.max(np.maximum(-path[i], path[i] - W))) / W for i in shapes.DIMS_FAR]
    assert all(1e3 <= v <= 1e4 for v in out)
    f = path[shapes.DIMS_LAST_AXIS]
    assert abs(f[D - 1]) > 1e3 * W and all(0.0 <= v <= W for v in f[:D - 1])
    far_verdicts = [v for (i, j), v in valid.items() if i in shapes.DIMS_FAR or j in shapes.DIMS_FAR]
    a, b = shapes.DIMS_TWINS
    assert b - a == 2 and np.array_equal(path[a], path[b]) and dist(a, b) == 0.0 and valid[(a, b)]
    print(name, c, "decided by a sphere >= 64 alone:", by_late_sphere, "by the inner box alone:", by_box,
          "far chords valid/invalid:", sum(far_verdicts), len(far_verdicts) - sum(far_verdicts))
    assert by_late_sphere >= 1 and by_box >= 1
    assert sum(far_verdicts) >= 1 and len(far_verdicts) - sum(far_verdicts) >= 100
    assert c["valid"] >= 100 and c["invalid"] >= 100


def test_bad_adjacent_r3_the_planners_edge_fails_check_motion():
    scene = shapes.bad_adjacent_r3()
    problem = scene["problems"][0]
    a, b = shapes.BAD_EDGE
    o = gen.rn_oracle(scene, problem)
    path = problem["path"]
    assert not o.check_motion(path[a], path[b])
    assert all(o.check_motion(path[k], path[k + 1]) for k in range(len(path) - 1) if k != a)
    idx = gen.result("bad_adjacent_r3", 0, 0)[0]
    print("bad_adjacent_r3 idx", idx)
    assert a in idx and idx[idx.index(a) + 1] == b          # the DP uses the edge that check_motion refuses
    c = census("bad_adjacent_r3", 0, 0)
    assert c["valid"] >= 1 and c["invalid"] >= 1


def test_so3_arc_signs_twins_switch_pair_and_both_verdicts():
    scene = shapes.so3_arc()
    path = scene["problems"][0]["path"]
    rows = [[float(v) for v in q] for q in path]
    L, valid, dist = gen.analysis("so3_arc", 0)
    assert L == shapes.SO3_L == 70 and len(scene["spheres"][1]) == 3
    assert all(abs(float(q @ q) - 1.0) < 1e-15 for q in path)
    assert all(so3.dot(rows[k], rows[k + 1]) < 0.0 for k in range(0, 8))       # neighbours stored with opposite signs
    a, b = shapes.SO3_TWINS
    assert np.array_equal(path[b], -path[a]) and dist(a, b) == 0.0
    a, b = shapes.SO3_SWITCH_PAIR
    d = abs(so3.dot(rows[a], rows[b]))
    assert 0.0 < 0.9995 - d < 1e-6
    c = census("so3_arc", 0, 0)
    print("so3_arc", c, "switch pair |dot| - 0.9995 =", d - 0.9995)
    assert c["valid"] >= 100 and c["invalid"] >= 100 and len(c["idx"]) >= 4


def test_full_tree_r2_fills_the_tree():
    scene = shapes.full_tree_r2()
    problem = scene["problems"][0]
    assert scene["max_nodes"] == len(problem["parents"]) == shapes.length(problem) == 1024
    assert problem["parents"].tolist() == [-1] + list(range(1023)) and problem["goal_node"] == 1023
    c = census("full_tree_r2", 0, 96)
    print("full_tree_r2 span 96", {k: v for k, v in c.items() if k != "idx"}, "waypoints", len(c["idx"]))
    assert c["valid"] >= 1000 and c["invalid"] >= 1000 and c["far"] >= 1


def _satisfied(scene, states, goal):
    centre = [float(v) for v in goal[0]]
    if scene["so3"]:
        return [so3.distance([float(v) for v in s], centre) <= goal[1] for s in states]
    from oracle import oracle_py as orc
    return [orc.distance(s, goal[0]) <= goal[1] for s in states]


@pytest.mark.parametrize("name", sorted(SCENES))
def test_planted_trees_give_their_paths_back(name):
    scene = SCENES[name]()
    for p, problem in enumerate(scene["problems"]):
        states, parents = problem["states"], problem["parents"]
        n = len(parents)
        assert n <= scene["max_nodes"] and parents[0] == -1 and all(0 <= parents[i] < i for i in range(1, n))
        exp = rh.expected(states, parents, np.ones(n, dtype=bool), _satisfied(scene, states, problem["goal"]))
        assert exp["n_removed"] == 0 and exp["goal_node"] == problem["goal_node"], (name, p)
        if problem["path"] is None:
            assert exp["goal_node"] == -1
            continue
        chain, v = [], exp["goal_node"]
        while v >= 0:
            chain.append(v)
            v = int(parents[v])
        chain.reverse()
        assert np.array_equal(states[chain].view(np.uint64), problem["path"].view(np.uint64)), (name, p)
        on_chain = set(chain)
        if n > len(chain):
            assert (np.diff(chain) > 1).any() and all(i not in on_chain for i in range(n) if i not in chain)
            decoys = [i for i in range(n) if i not in on_chain]
            assert any(int(parents[i]) in on_chain for i in decoys)


def test_golden_file_is_what_the_generator_writes_today():
    with open(gen.OUT) as f:
        committed = f.read()
    assert committed == gen.dumps(gen.build())
    data = json.loads(committed)
    assert sorted(k for k in data if not k.startswith("_")) == sorted(SCENES)
    assert os.path.getsize(gen.OUT) < 260000
    for name in ("corner_r2", "so3_arc", "bad_adjacent_r3") + tuple("dims_r%d" % D for D in shapes.DIMS):
        rec = data[name][0]
        bits = gen.unpack(rec["matrix"], len(gen.matrix_pairs(rec["L"])))
        assert int(bits.sum()) == rec["spans"]["0"]["valid"]
