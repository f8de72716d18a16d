"""CPU: the SO(3) PRM checker (tests/golden/make_golden_prm_so3.py) reproduces prm_so3_golden.json, its fixture path passes the
reference's own assertions (oxmpl/tests/prm_so3ss_tests.rs), and ox_acos stays inside the error bound the device's radius bands
rest on."""
import json
import math
import os
import random
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden as mg  # noqa: E402
import make_golden_prm_so3 as gp  # noqa: E402
import make_golden_so3 as g3  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "prm_so3_golden.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def runs():
    return {name: gp.run_scene(sc) for name, sc in gp.scenes().items()}


def test_checker_reproduces_the_golden_file(golden, runs):
    for name, sc in gp.scenes().items():
        rm, queries = runs[name]
        assert golden[name]["params"] == gp.scene_params(sc), name
        assert golden[name]["run"] == json.loads(json.dumps(gp.record(rm, queries))), name


def test_golden_covers_the_scenes_the_device_must_match(golden):
    assert golden["fixture"]["run"]["queries"][0]["status"] == "solved"
    assert golden["fixture"]["run"]["queries"][2]["status"] == "invalid_start"
    assert golden["tiny_radius"]["run"]["n"] > 100 and all(e == [] for e in golden["tiny_radius"]["run"]["edges"])
    wide = golden["wide_radius"]["run"]   # radius above PI / 2: every pair within it, check_motion decides
    assert 0 < sum(len(e) for e in wide["edges"]) < wide["n"] * (wide["n"] - 1)
    deg = golden["degenerate"]["run"]     # max_angle < 1e-9: every milestone is the centre, no word drawn, a complete graph
    assert deg["draws"] == 0 and len(set(map(tuple, deg["states"]))) == 1
    assert all(e == [j for j in range(deg["n"]) if j != i] for i, e in enumerate(deg["edges"]))
    cap = golden["sample_cap"]["run"]
    assert cap["n_samples"] == 150 and cap["n"] < 150


def test_fixture_path_passes_the_reference_assertions(runs):
    sc = gp.scenes()["fixture"]
    start, target, goal_r = sc["queries"][0]
    status, _, _, path = runs["fixture"][1][0]
    assert status == "solved" and path
    assert g3.distance(path[0], start) < 1e-9                           # "Path should start at the start state"
    assert g3.distance(path[-1], target) <= goal_r                      # "Path should end in the goal region"
    assert g3.is_so3_path_valid(path, g3.Cones(sc["cones"]), 0.05)      # is_path_valid


def test_ox_acos_is_within_the_band_margin_of_libm():
    """the radius bands assume |ox_acos(x) - acos(x)| <= 2^-52 acos(x) (below one ulp) with a margin of 2^-40; check 2^-50
    against libm's acos (itself within an ulp) on [0, 1 - 1e-9], dense near both ends"""
    rnd = random.Random(5)
    xs = [rnd.random() for _ in range(20000)] + [1.0 - 10 ** -rnd.uniform(1, 9) for _ in range(20000)]
    xs += [rnd.random() * 1e-3 for _ in range(5000)] + [0.0, 0.5, 1.0 - 1e-9, 2.0 ** -56, 2.0 ** -30]
    for x in xs:
        if x > 1.0 - 1e-9:
            continue
        a, b = g3.ox_acos(x), math.acos(x)
        assert abs(a - b) <= 2.0 ** -50 * b, (x, a, b)
    pio2 = 1.57079632679489655800e+00   # no distance exceeds fl(PI / 2): a radius above it takes every pair
    assert max(g3.ox_acos(x) for x in [0.0, 1e-300, 2.0 ** -60, 2.0 ** -55, 6e-17, 1e-16]) == pio2


def test_checker_n_samples_counts_sample_uniform_calls():
    """n_samples counts accepted attempts (sample_uniform calls); the stream moves 4 words per attempt"""
    rng = mg.ChaCha12Rng(1, 2)
    calls = 0
    for _ in range(50):
        g3.sample_uniform(rng, [0.0, 0.0, 0.0, 1.0], g3.PI)
        calls += 1
    assert rng.draws % 4 == 0 and rng.draws > 4 * calls
