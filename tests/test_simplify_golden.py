"""CPU: tests/golden/simplify_golden.json is what its generator derives today -- the shortcut of DESIGN.md section 18 (the DP of
tests/simplify_helpers.py) over the CPU oracle's own paths, check_motion and distance -- and its records have the properties the
semantics promise.  tests/test_gpu_simplify.py reproduces the same records on the device."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_simplify as gen  # noqa: E402
from helpers import unhex  # noqa: E402
import simplify_helpers as sh  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "simplify_golden.json")) as f:
        return json.load(f)


def test_the_file_is_compact_and_covers_what_it_should(golden):
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "simplify_golden.json")) < 16384
    assert [len(golden[k]) for k in ("config1", "config2", "wall", "config1_star", "so3_fixture")] == [8, 8, 8, 2, 4]
    assert golden["seed"] == sh.SEED


@pytest.mark.parametrize("scene", ["config1", "config2", "wall"])
def test_rn_records_are_rederived(golden, scene):
    assert gen.rn_records(sh.rn_scenes()[scene], range(gen.RN_PROBLEMS)) == golden[scene]


def test_rrt_star_records_are_rederived(golden):
    assert gen.rn_records(sh.rn_scenes()["config1"], range(gen.STAR_PROBLEMS), gen.STAR_RADIUS) == golden["config1_star"]


def test_so3_records_are_rederived(golden):
    assert gen.so3_records(range(gen.SO3_PROBLEMS)) == golden["so3_fixture"]


def test_every_record_keeps_the_promises_of_the_semantics(golden):
    n = 0
    for key, recs in golden.items():
        if not isinstance(recs, list):
            continue
        for rec in recs:
            L = rec["L"]
            for span, r in rec["spans"].items():
                idx = r["idx"]
                assert idx[0] == 0 and idx[-1] == L - 1 and all(a < b for a, b in zip(idx, idx[1:]))
                assert all(b - a <= sh.span_of(L, int(span)) for a, b in zip(idx, idx[1:]))
                assert unhex(r["cost"]) <= unhex(r["raw"])          # exactly: the raw chain is a candidate
                assert r["checks"] == sh.expected_checks(L, int(span))
                n += 1
            assert rec["spans"]["0"]["raw"] == rec["spans"]["3"]["raw"]
            assert unhex(rec["spans"]["0"]["cost"]) <= unhex(rec["spans"]["3"]["cost"])
    assert n == 60
