"""CPU: tests/golden/prm_shortest_golden.json is what its generator -- the pure-Python checker of oxhip_prm_solve_batch_shortest
 -- computes today, and it says what it is meant to say: on the 32 queries of each scene of
prm_batch_golden.json the statuses are the breadth-first batch's, every recorded path's left-to-right cost equals its label bit
for bit and is no more than the BFS path's, the unit-weight paths have BFS's length, and the mix is the one recorded in the issue
(solved 31 / 11 / 23, paths that differ from BFS's 29 / 6 / 23), so the file cannot pass on nothing."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_prm_shortest as gsp  # noqa: E402

SCENES = ("wall", "r6", "fixture")


def _golden(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def rebuilt():
    """the three roadmaps and all 96 queries again, in pure Python, once (about ten seconds)"""
    return gsp.build_scenes()


def test_checker_reproduces_the_golden_file(rebuilt):
    out, _ = rebuilt
    want = _golden("prm_shortest_golden.json")
    assert json.loads(json.dumps(out)) == want
    assert os.path.getsize(os.path.join(HERE, "golden", "prm_shortest_golden.json")) < (1 << 20)
    for scene in SCENES:
        assert len(want[scene]["queries"]) == 32


@pytest.mark.parametrize("scene", SCENES)
def test_recorded_paths_cost_their_label_and_no_more_than_bfs(rebuilt, scene):
    _, kept = rebuilt
    states, dist = kept[scene]
    recs, bfs = _golden("prm_shortest_golden.json")[scene]["queries"], _golden("prm_batch_golden.json")[scene]["queries"]
    solved, differ, ratio = gsp.check_against_bfs(recs, bfs, states, dist)
    assert solved == {"wall": 31, "r6": 11, "fixture": 23}[scene]
    assert differ == {"wall": 29, "r6": 6, "fixture": 23}[scene]
    assert ratio > 1.0
    for r in recs:
        if r["status"] == "solved":
            assert len(r["nodes"]) >= len(r["nodes_unit"]) >= 1       # unit weights give the fewest hops
