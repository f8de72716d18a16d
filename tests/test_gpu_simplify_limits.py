"""-m gpu: path extraction and shortcutting (path_simplify.hip) on the planted paths of
tests/simplify_limits_shapes.py: DP windows wider than the wave, exact ties, R^2 .. R^8 and SO(3), more than 64 spheres with boxes, states
far outside the bounds, chords of length zero, slot counts around a 64-bit word, mixed rounds, a tree filled to max_nodes.

Planting: a batch without obstacles, setup, set_tree per problem, revalidate_trees() -- which removes nothing and sets goal_node to the
lowest index >= 1 that satisfies the goal -- then the obstacles, then extract_paths.

Every comparison is bit for bit or exact.  Yardsticks: the planted rows for the extraction; RRTBatch.check_motion (one call per problem)
and tests/golden/simplify_limits.json (the CPU oracle's verdicts) for the pair matrix; the golden records and the Python DP of
tests/simplify_helpers.py over check_motion and distance_batch / so3_op_batch for whole results."""
import json
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from oxmpl_amd import capi  # noqa: E402
from helpers import bits, unhex  # noqa: E402
import simplify_helpers as sh  # noqa: E402
import simplify_limits_shapes as shapes  # noqa: E402

pytestmark = pytest.mark.gpu

SCENES = shapes.scenes()
_PLANTED = {}
_PAIRS = {}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "simplify_limits.json")) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------ planting (once per scene)

def planted(name):
    """the scene's batch with its trees planted, its obstacles set and its paths extracted"""
    if name in _PLANTED:
        return _PLANTED[name]
    scene = SCENES[name]()
    probs = scene["problems"]
    P = len(probs)
    if scene["so3"]:
        g = capi.RRTBatch(4, [0.0, 0.0, 0.0, 1.0, math.pi], 0.3, 0.05, P, scene["max_nodes"], scene["lvs_fraction"], False, 7,
                          space=capi.SPACE_SO3)
    else:
        g = capi.RRTBatch(scene["dim"], scene["bounds"], 0.5, 0.05, P, scene["max_nodes"], scene["lvs_fraction"], False, 7)
    g.setup(np.array([q["states"][0] for q in probs]), np.array([q["goal"][0] for q in probs]), np.array([q["goal"][1] for q in probs]))
    for p, q in enumerate(probs):
        g.set_tree(p, q["states"], q["parents"])
    r = g.revalidate_trees()                                  # no obstacle yet: nothing goes, the goal nodes are found from the states
    assert not r["n_removed"].any() and not r["goal_lost"].any()
    c = g.counts()
    assert c["goal_node"].tolist() == [q["goal_node"] for q in probs]
    assert c["nodes"].tolist() == [len(q["parents"]) for q in probs]
    if len(scene["spheres"][1]):
        g.set_spheres(*scene["spheres"])
    if scene["boxes"] is not None:
        g.set_boxes(*scene["boxes"])
    assert g.counts()["goal_node"].tolist() == [q["goal_node"] for q in probs]
    g.extract_paths()
    _PLANTED[name] = (scene, g)
    return scene, g


def _distance(g, a, b):
    if g.space == capi.SPACE_SO3:
        return capi.so3_op_batch(0, a, b)
    return capi.distance_batch(a, b)


def pairs(name, p):
    """(valid {(i, j)}, dist {(i, j)}) over every pair i < j of problem p's planted path: one check_motion call, one distance call"""
    if (name, p) not in _PAIRS:
        scene, g = planted(name)
        path = scene["problems"][p]["path"]
        L = shapes.length(scene["problems"][p])
        S = max(sh.span_of(L, s) for s in shapes.spans_of(name, scene, p)) if L else 0
        if L < 2:
            _PAIRS[(name, p)] = ({}, {})
        else:
            ii, jj = np.triu_indices(L, 1)
            keep = (jj - ii) <= S
            ii, jj = ii[keep], jj[keep]
            keys = list(zip(ii.tolist(), jj.tolist()))
            _PAIRS[(name, p)] = (dict(zip(keys, g.check_motion(path[ii], path[jj]).tolist())),
                                 dict(zip(keys, _distance(g, path[ii], path[jj]).tolist())))
    return _PAIRS[(name, p)]


def model(name, p, span):
    scene, _ = planted(name)
    L = shapes.length(scene["problems"][p])
    valid, dist = pairs(name, p)
    return sh.shortcut_dp(L, lambda i, j: valid[(i, j)], lambda i, j: dist[(i, j)], span)


def results(g, span, chunk=0):
    g.simplify_paths(span, chunk)
    off, rows, idx, raw, simp, checks = g.simplified_paths()
    return dict(off=off, rows=rows, idx=idx, raw=raw, simp=simp, checks=checks)


def assert_problem(r, p, want, path, tag):
    """r: results of the batch; want: (idx, raw, cost, checks)"""
    idx, raw, cost, checks = want
    a, b = int(r["off"][p]), int(r["off"][p + 1])
    assert r["idx"][a:b].tolist() == idx, tag
    assert bits(r["raw"][p]) == bits(raw) and bits(r["simp"][p]) == bits(cost), tag
    assert int(r["checks"][p]) == checks, tag
    if idx:
        assert np.array_equal(bits(r["rows"][a:b]), bits(path[idx])), tag
    else:
        assert a == b and r["raw"][p] == 0.0 and r["simp"][p] == 0.0, tag


def golden_want(rec, span):
    w = rec["spans"][str(span)]
    return w["idx"], unhex(w["raw"]), unhex(w["cost"]), w["checks"]


def golden_matrix(rec):
    """[L][L] bool from the golden record's row-major bits of the pairs j - i >= 2"""
    L = rec["L"]
    n = (L - 1) * (L - 2) // 2
    flat = np.unpackbits(np.frombuffer(bytes.fromhex(rec["matrix"]), dtype=np.uint8))[:n].astype(bool)
    M = np.zeros((L, L), dtype=bool)
    M[np.triu_indices(L, 2)] = flat
    return M


# ------------------------------------------------------------------------------------------------ extraction

@pytest.mark.parametrize("name", sorted(SCENES))
def test_extraction_returns_the_planted_rows(name):
    scene, g = planted(name)
    off, rows = g.paths()
    lengths = [shapes.length(q) for q in scene["problems"]]
    assert off.tolist() == np.concatenate([[0], np.cumsum(lengths)]).tolist() and len(rows) == sum(lengths)
    for p, q in enumerate(scene["problems"]):
        got = rows[int(off[p]):int(off[p + 1])]
        ref = g.path(p)
        assert got.shape == ref.shape == (lengths[p], g.dim), (name, p)
        assert np.array_equal(bits(got), bits(ref)), (name, p)
        if lengths[p]:
            assert np.array_equal(bits(got), bits(q["path"])), (name, p)


# ------------------------------------------------------------------------------------------------ the pair matrix

@pytest.mark.parametrize("name", sorted(SCENES))
def test_pair_matrix_is_check_motions_verdict_and_the_oracles(name, golden):
    scene, g = planted(name)
    seen = set()
    for p, q in enumerate(scene["problems"]):
        L = shapes.length(q)
        rec = golden[name][p]
        assert rec["L"] == L
        if L < 2:
            continue
        valid, _ = pairs(name, p)
        spans = shapes.spans_for(L) if name != "full_tree_r2" else (96, 65, 2)   # (the 1024-state path: within the span its tests run)
        for span in spans:
            M = g.path_valid_matrix(p, span)
            S = sh.span_of(L, span)
            assert M.shape == (L, L)
            ii, jj = np.triu_indices(L, 2)
            keep = (jj - ii) <= S
            want = np.array([valid[ij] for ij in zip(ii[keep].tolist(), jj[keep].tolist())], dtype=bool)
            assert np.array_equal(M[ii[keep], jj[keep]], want), (name, p, span)
            assert M[np.arange(L - 1), np.arange(1, L)].all()                     # adjacent: true without a check
            assert not M[ii[~keep], jj[~keep]].any() and not np.tril(M).any()     # beyond the span, and the lower triangle
            if str(span) in rec["spans"]:
                assert int(want.sum()) == rec["spans"][str(span)]["valid"], (name, p, span)
            if "matrix" in rec:
                G = golden_matrix(rec)
                assert np.array_equal(M[ii[keep], jj[keep]], G[ii[keep], jj[keep]]), (name, p, span)
            seen.update(want.tolist())
    assert seen == {True, False} or name == "line_free_r2"


# ------------------------------------------------------------------------------------------------ whole results

@pytest.mark.parametrize("name", sorted(set(SCENES) - {"mixed_batch"}))
def test_dp_equals_the_golden_record_and_the_model(name, golden):
    scene, g = planted(name)
    spans = sorted(set(s for p in range(len(scene["problems"])) for s in shapes.spans_of(name, scene, p)))
    for span in spans:
        r = results(g, span)
        for p, q in enumerate(scene["problems"]):
            if span not in shapes.spans_of(name, scene, p):
                continue
            want = model(name, p, span)
            assert_problem(r, p, want, q["path"], (name, p, span, "model"))
            assert_problem(r, p, golden_want(golden[name][p], span), q["path"], (name, p, span, "golden"))
            assert want[3] == sh.expected_checks(shapes.length(q), span)


@pytest.mark.parametrize("name, p", [("corner_r2", 0), ("arc_r2", shapes.ARC_LENGTHS.index(shapes.ARC_SPANS_L))])
def test_spans_around_the_wave_and_the_path_length(name, p):
    scene, g = planted(name)
    path = scene["problems"][p]["path"]
    L = len(path)
    assert L == 200
    out = {}
    for span in (1, 2, 63, 64, 65, L - 2, L - 1, L, 2 ** 32 - 1):
        r = results(g, span)
        assert_problem(r, p, model(name, p, span), path, (name, span))
        a, b = int(r["off"][p]), int(r["off"][p + 1])
        out[span] = (r["idx"][a:b].tolist(), bits(r["raw"][p]).item(), bits(r["simp"][p]).item(), int(r["checks"][p]))
    assert out[L - 1] == out[L] == out[2 ** 32 - 1]
    assert out[L - 2] != out[L - 1]                                       # (one pair more: the checks differ at least)
    assert out[1][0] == list(range(L)) and out[1][1] == out[1][2] and out[1][3] == 0
    if name == "corner_r2":
        assert out[L - 1][0] == [0, 98, 100, 199]


def test_line_free_parents_are_the_window_start():
    scene, g = planted("line_free_r2")
    for span in (0, 65):
        r = results(g, span)
        for p, L in enumerate(shapes.LINE_LENGTHS):
            S = sh.span_of(L, span)
            a, b = int(r["off"][p]), int(r["off"][p + 1])
            want = list(range((L - 1) % S, L, S))
            assert r["idx"][a:b].tolist() == ([0] + want if want[0] else want), (span, L)
            assert r["simp"][p] == r["raw"][p] == 0.25 * (L - 1)


def test_mixed_batch_under_every_round_size(golden):
    scene, g = planted("mixed_batch")
    P = len(scene["problems"])
    for span in scene["spans"]:
        ref = results(g, span, 0)
        assert g.paths_last_timing()["rounds"] == 1
        for p, q in enumerate(scene["problems"]):
            assert_problem(ref, p, model("mixed_batch", p, span), q["path"], (p, span, "model"))
            assert_problem(ref, p, golden_want(golden["mixed_batch"][p], span), q["path"], (p, span, "golden"))
        for chunk in shapes.MIXED_CHUNKS[1:]:
            got = results(g, span, chunk)
            assert g.paths_last_timing()["rounds"] == -(-P // chunk)
            for k in ref:
                assert np.array_equal(bits(ref[k]) if ref[k].dtype == np.float64 else ref[k],
                                      bits(got[k]) if got[k].dtype == np.float64 else got[k]), (span, chunk, k)


def test_full_tree_every_node_on_the_path():
    scene, g = planted("full_tree_r2")
    assert g.max_nodes == 1024 and int(g.counts()["nodes"][0]) == 1024
    off, rows = g.paths()                                   # (a corrupt-tree report would have failed extract_paths)
    assert off.tolist() == [0, 1024] and np.array_equal(bits(rows), bits(scene["problems"][0]["path"]))
    r = results(g, 96)
    want = model("full_tree_r2", 0, 96)
    assert_problem(r, 0, want, scene["problems"][0]["path"], "span 96")
    assert len(want[0]) < 1024 // 8


def test_bad_adjacent_edge_is_kept_as_the_planners():
    scene, g = planted("bad_adjacent_r3")
    path = scene["problems"][0]["path"]
    a, b = shapes.BAD_EDGE
    assert not g.check_motion(path[a][None], path[b][None])[0]
    assert g.path_valid_matrix(0)[a, b]
    r = results(g, 0)
    idx = model("bad_adjacent_r3", 0, 0)[0]
    assert r["idx"].tolist() == idx
    assert a in idx and idx[idx.index(a) + 1] == b

