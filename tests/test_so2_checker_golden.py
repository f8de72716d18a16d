"""CPU: the SO(2) checker (tests/golden/make_golden_so2.py) against its golden file, against the oracle's restatement of the same
arithmetic (oracle/se2_oracle.c: orc_so2_*) bit for bit, and against the reference's own assertions on every golden path."""
import ctypes as C
import math

import numpy as np
import pytest

import so2_helpers as h
from so2_helpers import so2
from oracle import oracle_py as orc


@pytest.fixture(scope="module")
def golden():
    return h.load_golden()


SCENES = ["fixture", "bounded", "bias1", "blocked", "tiny"]


@pytest.mark.parametrize("scene", SCENES)
def test_checker_reproduces_the_golden_file(golden, scene):
    sc = so2.scenes()[scene]
    assert so2.scene_params(sc) == golden[scene]["params"]
    assert [(r["seed"], r["pid"]) for r in golden[scene]["runs"]] == [(0, 0), (7, 3)]
    for run in golden[scene]["runs"]:
        rec = so2.record(so2.run_scene(sc, run["seed"], run["pid"]))
        rec.update(seed=run["seed"], pid=run["pid"])
        assert rec == run


def _inputs():
    rng = np.random.default_rng(12)
    PI = so2.PI
    special = []
    for c in (PI, -PI, 0.0, -0.0, 2.0 * PI, -2.0 * PI, 4.0 * PI, -4.0 * PI, 3.0 * PI):
        special += [c, float(np.nextafter(c, 10.0)), float(np.nextafter(c, -10.0)), c + 1e-9, c - 1e-9]
    a = np.concatenate([rng.uniform(-PI, PI, 4000), rng.uniform(-7.0, 7.0, 3000), rng.uniform(-13.0, 13.0, 1500),
                        rng.uniform(-1e6, 1e6, 1000), rng.uniform(-1e15, 1e15, 300), special])   # the window and the fmod branch
    b = np.concatenate([rng.uniform(-PI, PI, 4000), rng.uniform(-7.0, 7.0, 3000), rng.uniform(-13.0, 13.0, 1500),
                        rng.uniform(-1e6, 1e6, 1000), rng.uniform(-1e15, 1e15, 300), rng.permutation(special)])
    anti = rng.uniform(-PI, PI, 400)
    a = np.concatenate([a, anti, anti, special])
    b = np.concatenate([b, anti + PI, anti - PI, special])            # antipodal pairs, equal pairs
    t = rng.random(a.size)
    t[::5] = 0.0
    t[2::5] = 1.0
    return a.tolist(), b.tolist(), t.tolist()


def test_arithmetic_equals_the_oracles_bit_for_bit():
    L = orc.lib()
    a, b, t = _inputs()
    assert len(a) >= 10000
    bits = lambda v: np.float64(v).view(np.uint64)  # noqa: E731
    for x, y, tt in zip(a, b, t):
        assert bits(so2.normalise(x)) == bits(L.orc_so2_normalise(x)), x
        assert bits(so2.distance(x, y)) == bits(L.orc_so2_distance(x, y)), (x, y)
        assert bits(so2.interpolate(x, y, tt)) == bits(L.orc_so2_interpolate(x, y, tt)), (x, y, tt)


@pytest.mark.parametrize("scene", SCENES)
def test_golden_paths_pass_the_reference_assertions(golden, scene):
    sc = h.scene_from_params(golden[scene]["params"])
    for run in golden[scene]["runs"]:
        r = h.run_from_record(run)
        if r["goal_node"] < 0:
            assert r["path"] == []
            continue
        h.reference_path_assertions(r["path"], sc)
        assert r["path"][-1] == r["states"][r["goal_node"]] and r["path"][0] == r["states"][0]


def test_what_the_scenes_are_for(golden):
    for run in golden["fixture"]["runs"]:
        path = h.run_from_record(run)["path"]
        assert any(abs(x - y) > so2.PI for x, y in zip(path, path[1:]))       # a step across the +-PI seam
    assert so2.mg.num_steps(0.2, so2.lvsl(0.05)) == 13                        # states per full step of the fixture
    for run in golden["blocked"]["runs"]:
        assert run["accepted"] == 0 and run["n"] == 1 and run["goal_node"] == -1
    for run in golden["bias1"]["runs"]:
        assert run["rng_draws"] == 0                                          # goal_bias 1: no Bernoulli word, no range draw
    for scene in ("fixture", "bounded", "tiny"):
        assert all(run["goal_node"] >= 0 for run in golden[scene]["runs"])
    assert math.pi == so2.PI
