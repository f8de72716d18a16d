"""CPU: tests/golden/prm_revalidate.json (make_golden_prm_revalidate.py, pure Python) against a second derivation.  The fixture
holds no roadmap, only checksums, the invalid indices and sizes: the R^n roadmaps are rebuilt here by the C oracle's PRM (and must
show the fixture's checksums), the SO(3) one by the generator itself.

R^n scenes: every verdict -- valid[i] per milestone, check_motion(from = j, to = i) per edge {i < j} between two valid milestones
-- is re-derived with the C oracle's is_valid / check_motion, reached through OracleRRT (oracle_py).  The oracle's PRM and RRT
motion checks are the same arithmetic: oracle/prm_oracle.c:147-162 and oracle/rrt_oracle.c:372-389 are the same loop over
orc_distance / orc_maximum_extent / orc_num_steps / orc_interpolate, and both validity tests are distance(centre, s) > radius per
sphere and lo <= s <= hi per box ("the same loop in all three").  SO(3) has no C oracle: it is compared with
the Python restatement only, i.e. the generator's scene is run again and must reproduce the record (about ten seconds).

The direction record: the generator found a pair (a, b), both valid, whose motion a -> b is invalid and b -> a valid (after 70
grazing pairs); the oracle must agree with both verdicts."""
import os
import sys

import numpy as np
import pytest

from helpers import unhex
from prm_helpers import csr_checksum, make_oracle_prm, states_checksum
from prm_revalidate_helpers import added_spheres, csr, edge_lists, fixture, plain_filter, unhex_rows, valid_mask

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))


def _oracle_rrt(P, extra_c, extra_r, extra_boxes):
    from oracle import oracle_py as orc
    dim = P["dim"]
    o = orc.OracleRRT(dim, P["bounds"], 1.0, 0.05, lvs_fraction=P["fraction"])
    c = [[unhex(v) for v in cc] for cc, _ in P["spheres"]] + [list(row) for row in extra_c]
    r = [unhex(rr) for _, rr in P["spheres"]] + list(extra_r)
    if r:
        o.set_spheres(c, r)
    boxes = list(P["boxes"]) + list(extra_boxes)
    if boxes:
        o.set_boxes([lo for lo, _ in boxes], [hi for _, hi in boxes])
    o.setup([0.0] * dim, [1.0] * dim, 0.1)   # (check_motion answers only after setup, rrt.rs:113-115)
    return o


@pytest.mark.parametrize("name", ["r2_radius", "r2_small", "r6_knn"])
def test_rn_verdicts_equal_the_c_oracle(name):
    sc = fixture()[name]
    P = sc["params"]
    prm = make_oracle_prm(P)
    prm.setup([0.5] * P["dim"], [9.5] * P["dim"], 0.5)
    prm.construct_roadmap(P["max_milestones"])
    states, off, nbrs = prm.roadmap()
    lists = edge_lists(off, nbrs)
    assert len(states) == sc["n"] and len(nbrs) == sc["entries_before"]
    assert "%016x" % states_checksum(states) == sc["states_checksum"]
    assert "%016x" % csr_checksum(off, nbrs) == sc["csr_checksum_before"]
    c, r = added_spheres(sc)
    o = _oracle_rrt(P, c, r, sc["added"]["boxes"])
    valid = [o.is_valid(s) for s in states]
    assert np.array_equal(valid, valid_mask(sc)) and valid.count(False) == sc["n_invalid"] > 0
    ok = {(j, i): o.check_motion(states[j], states[i]) for j, row in enumerate(lists) for i in row if i < j and valid[i] and valid[j]}
    assert list(ok.values()).count(False) == sc["cut_between_valid"] > 0   # edges between two valid milestones go
    kept = plain_filter(lists, valid, ok)
    for u, row in enumerate(kept):
        assert row == sorted(set(row)) and u not in row and all(u in kept[v] for v in row) and (valid[u] or not row)
    assert "%016x" % csr_checksum(*csr(kept)) == sc["csr_checksum_after"] and kept == sc.get("edges_after", kept)
    assert sum(map(len, kept)) == sc["entries_after"] > 0 and sc["entries_before"] - sc["entries_after"] == sc["removed_entries"]


def test_so3_record_equals_the_python_restatement():
    import make_golden_prm_revalidate as gen
    assert gen.scenes(only="so3")["so3"] == fixture()["so3"]


def test_direction_pair_differs_by_direction_in_the_oracle_too():
    d = fixture()["direction"]
    assert d["found"] and d["a_to_b"] is False and d["b_to_a"] is True
    a, b = unhex_rows([d["a"], d["b"]])
    P = dict(dim=2, bounds=d["bounds"], fraction=d["fraction"], spheres=[], boxes=[])
    o = _oracle_rrt(P, unhex_rows([d["sphere"][0]]), [unhex(d["sphere"][1])], [])
    assert o.is_valid(a) and o.is_valid(b)
    assert o.check_motion(a, b) is False and o.check_motion(b, a) is True
