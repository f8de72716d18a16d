"""-m gpu: RRT over SO2StateSpace (OXHIP_SPACE_SO2, rrt_so2.hip) against the CPU checker (tests/golden/make_golden_so2.py) and its
golden file, bit for bit: trees, parents, counts, checksums, goal nodes and paths -- on the reference's own fixture
(oxmpl/tests/rrt_so2ss_tests.rs), on varied scenes, across batch sizes, launch cuts (which pin the stream position a launch
leaves: it is what the next one starts from), freeze and a bounded fuzz leg -- the checker's entry points, and the Python surface
on the fixture.  The arithmetic is add, subtract, multiply, divide and fmod: only the RNG stream is this build's own."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import so2_helpers as h  # noqa: E402
from so2_helpers import so2  # noqa: E402
from oxmpl_amd import capi  # noqa: E402


@pytest.fixture(scope="module")
def so2_golden():
    return h.load_golden()


@pytest.mark.parametrize("scene", ["fixture", "bounded", "bias1", "blocked", "tiny"])
def test_golden_cases_match_exactly(so2_golden, scene):
    sc = h.scene_from_params(so2_golden[scene]["params"])
    for run in so2_golden[scene]["runs"]:
        g = h.make_gpu(sc, 1, run["seed"], run["pid"])
        st = g.solve(sc["max_iterations"])
        assert (st[0] == capi.OK) == (run["goal_node"] >= 0)
        h.assert_same(g, 0, h.run_from_record(run))
        g.close()


def test_stream_kernel_kind_runs_the_same_kernel(so2_golden):
    sc = h.scene_from_params(so2_golden["fixture"]["params"])
    run = so2_golden["fixture"]["runs"][0]
    g = h.make_gpu(sc, 1, run["seed"], run["pid"], kernel=capi.KERNEL_STREAM)
    g.solve(sc["max_iterations"])
    h.assert_same(g, 0, h.run_from_record(run))


@pytest.fixture(scope="module")
def fixture_1024():
    sc = so2.fixture_scene()
    g = h.make_gpu(sc, 1024, 42, 0)
    st = g.solve(2000)
    return sc, g, st


def test_1024_fixture_problems_against_the_checker(fixture_1024):
    sc, g, st = fixture_1024
    assert (st == capi.OK).all()
    c = g.counts()
    for p in range(32):
        h.assert_same(g, p, so2.run_scene(sc, 42, p, max_iterations=2000), c)


def test_1024_fixture_paths_pass_the_reference_assertions_and_cross_the_seam(fixture_1024):
    sc, g, _ = fixture_1024
    for p in range(1024):
        path = g.path(p).reshape(-1).tolist()
        h.reference_path_assertions(path, sc)
        assert any(abs(a - b) > h.PI for a, b in zip(path, path[1:])), p   # the arc blocks the direct way: through +-PI


def test_problem_0_across_batch_sizes_and_launch_cuts(fixture_1024):
    sc, g, _ = fixture_1024
    want = so2.run_scene(sc, 42, 0, max_iterations=2000)
    h.assert_same(g, 0, want)
    for n_problems, cut in ((1, None), (64, None), (3, 1), (3, 7), (3, 64)):
        g1 = h.make_gpu(sc, n_problems, 42, 0)
        if cut is None:
            g1.solve(2000)
        else:
            for _ in range(0, want["iterations"] + cut, cut):   # every call resumes at the stream position the last one left
                g1.solve(cut)
        h.assert_same(g1, 0, want)
        g1.close()


def test_growth_without_stopping_across_cuts():
    """stop_at_goal = 0: 300 iterations in one launch, and cut at 1, 7, 64 and 100 (inside a sampled block)"""
    sc = h.scene(max_distance=0.05, goal_bias=0.1, start=1.0, target=1.6, arcs=[(0.2, 0.4), (-2.9, -2.7)])
    want = so2.run_scene(sc, 5, 11, max_iterations=300, stop_at_goal=False)
    assert want["goal_node"] >= 0 and want["n"] > want["goal_node"] + 10   # it went on after the goal
    for cut in (300, 1, 7, 64, 100):
        g = h.make_gpu(sc, 2, 5, 11, stop_at_goal=False)
        left = 300
        while left:
            g.solve(min(cut, left))
            left -= min(cut, left)
        h.assert_same(g, 0, want)
        g.close()


def test_freeze_counts_without_growing():
    sc = so2.fixture_scene()
    grown = so2.run_scene(sc, 9, 2, max_iterations=20)
    g = h.make_gpu(sc, 4, 9, 0)
    g.solve(20)
    h.assert_same(g, 2, grown)
    g.solve(100, freeze=True)
    # the checker from the same tree, at the stream position and checksum the growing run left
    want = so2.rrt_solve(sc["bounds"], sc["max_distance"], sc["goal_bias"], sc["fraction"], so2.Arcs(sc["arcs"]), sc["start"],
                         sc["target"], sc["goal_r"], 9, 2, 100, sc["max_nodes"], freeze=True, tree=grown["states"],
                         parents=grown["parents"], draws=grown["rng_draws"])
    c = g.counts()
    assert int(c["nodes"][2]) == grown["n"] and int(c["iterations"][2]) == 20 + want["iterations"]
    assert int(c["accepted"][2]) == grown["accepted"] + want["accepted"]
    gs, gp = g.tree(2)
    assert np.array_equal(h.bits(gs).reshape(-1), h.bits(np.array(grown["states"])))
    # the checksum continues the polynomial: H * P^m + (the frozen run's polynomial from a zero basis)
    M64, P = so2.M64, so2.mg.FNV_P
    frozen_from_zero = (want["checksum"] - so2.mg.FNV_BASIS * pow(P, want["iterations"], 1 << 64)) & M64
    assert int(c["checksum"][2]) == (grown["checksum"] * pow(P, want["iterations"], 1 << 64) + frozen_from_zero) & M64


def test_fuzz_leg():
    rng = np.random.default_rng(20)
    for case in range(30):
        lo = float(rng.uniform(-3.0, 0.5))
        hi = float(lo + rng.uniform(0.5, 7.0))
        bounds = None if case % 5 == 0 else (lo, hi)
        clo, chi = so2.space_bounds(bounds)
        arcs = []
        for _ in range(int(rng.integers(0, 6))):
            a = float(rng.uniform(-h.PI, h.PI))
            arcs.append((a, a + float(rng.uniform(0.01, 0.4))))
        sc = h.scene(bounds=bounds, max_distance=float(rng.choice([0.01, 0.1, 0.3, 1.0, 4.0])),
                     goal_bias=float(rng.choice([0.0, 0.05, 0.5, 1.0])), fraction=float(rng.choice([0.01, 0.05, 0.3, 1.0, 2.0])),
                     start=float(rng.uniform(clo, chi)), target=float(rng.uniform(clo, chi)), goal_r=float(rng.uniform(0.01, 0.3)),
                     arcs=arcs, max_nodes=int(rng.choice([40, 300])), max_iterations=150)
        seed, pid = int(rng.integers(0, 1 << 40)), int(rng.integers(0, 1 << 20))
        g = h.make_gpu(sc, 2, seed, pid)
        g.solve(100)
        g.solve(50)
        for p in range(2):
            h.assert_same(g, p, so2.run_scene(sc, seed, pid + p, max_iterations=150))
        g.close()


def test_is_valid_and_check_motion_rows():
    rng = np.random.default_rng(8)
    arcs = [(-0.5, 0.5), (2.9, 3.2), (-3.2, -3.0), (1.0, 1.0)]
    sc = h.scene(arcs=arcs, fraction=0.05)
    g = h.make_gpu(sc, 1, 0, 0)
    ck = so2.Arcs(arcs)
    ends = np.array([v for lo, hi in arcs for v in (lo, hi)])
    edge = np.concatenate([np.nextafter(ends, -10.0), ends, np.nextafter(ends, 10.0), [h.PI, -h.PI, 0.0, -0.0, 2 * h.PI, 7.0, -9.0, 50.0]])
    states = np.concatenate([rng.uniform(-7.0, 7.0, 10000), edge])
    got = g.is_valid(states.reshape(-1, 1))
    assert np.array_equal(got.astype(bool), np.array([ck.is_valid(v) for v in states.tolist()]))
    frm = np.concatenate([rng.uniform(-7.0, 7.0, 8000), rng.uniform(-h.PI, h.PI, 2000)])
    to = np.concatenate([rng.uniform(-7.0, 7.0, 8000), frm[8000:] + rng.uniform(-0.03, 0.03, 2000)])
    got = g.check_motion(frm.reshape(-1, 1), to.reshape(-1, 1))
    want = np.array([so2.check_motion(ck, sc["fraction"], a, b) for a, b in zip(frm.tolist(), to.tolist())])
    assert np.array_equal(got.astype(bool), want)
    assert want.any() and not want.all()


def test_python_surface_solves_the_fixture():
    from oxmpl_amd import scenarios
    from oxmpl_amd.base import ProblemDefinition, SO2ArcValidityChecker, SO2State, SO2StateSpace
    from oxmpl_amd.geometric import RRT

    class Goal:
        target, radius = SO2State(math.pi / 2.0), 0.1

    space = SO2StateSpace()
    pd = ProblemDefinition.from_so2(space, SO2State(-math.pi / 2.0), Goal())
    planner = RRT(0.2, 0.05, pd, seed=0, problem_id=0)
    checker = SO2ArcValidityChecker([(-0.5, 0.5)])
    planner.setup(checker)
    path = planner.solve(5.0)
    run = h.run_from_record(h.load_golden()["fixture"]["runs"][0])
    assert [s.value for s in path.states] == run["path"]
    assert all(isinstance(s, SO2State) for s in path.states)
    assert space.distance(path.states[0], SO2State(-math.pi / 2.0)) < 1e-9 and space.distance(path.states[-1], Goal.target) <= 0.1
    short = planner.simplify_solution()
    assert 2 <= len(short) <= len(path) and short.states[0] == path.states[0] and short.states[-1] == path.states[-1]
    assert planner.is_state_valid(SO2State(1.0)) and not planner.is_state_valid(SO2State(0.25))
    removed = planner.revalidate(SO2ArcValidityChecker([(-0.5, 0.5), (2.0, 2.2)]))   # the arc cuts the found path
    assert removed > 0 and planner.num_nodes == run["n"] - removed
    sc = scenarios.so2_band()
    b = scenarios.make_so2_batch(sc, 1, seed=0)
    b.solve(20000)
    h.assert_same(b, 0, run)
