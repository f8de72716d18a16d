"""-m gpu: rejected range draws in the lane-parallel sampler (oxmpl_amd/csrc/lane_sampler.hpp) and its sequential fallback.

rand's random_range draws again when v01 * scale + lo rounds up to hi.  With ordinary bounds that happens once in ~2^53 draws, so
no other RRT test ever reaches the "one by one" fallback of the block samplers, nor the fast-forward of a split frozen launch
across a rejected draw.  Here the x bounds are [2^50, 2^50 + 8): one ulp is 0.25 there and v01 * 8 + 2^50 rounds up to hi for
about one draw in 64, so every problem meets several rejections in 512 iterations -- some blocks of 64 iterations hold one (the
fallback runs) and some hold none (the lane-parallel path runs).  A box wall keeps the problems unsolved for all 512 iterations.
That every problem does meet a rejection is asserted from a replay of its stream with the golden generator's own RNG
(tests/golden/make_golden.py), independently of the oracle and of the device.

Every kernel that samples blocks of iterations is compared with the CPU oracle bit for bit, as tests/test_gpu_parity.py compares;
the streaming kernel, which samples one by one, is the control that shows the scene itself agrees.  The stream position
(ProblemState::draws) is not readable through the C ABI: it is what a further launch starts from, so each case runs 64 more
iterations after the 512 and compares again."""
import functools
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden as mg  # noqa: E402

from helpers import bits  # noqa: E402
from oxmpl_amd import capi, scenarios  # noqa: E402
from oracle import oracle_py as orc  # noqa: E402

X0 = 2.0 ** 50
SEED, P, MAX_NODES, ITERS, MORE = 21, 4, 1024, 512, 64


def scene(dim, goal_bias=0.05):
    return dict(dim=dim, bounds=[(X0, X0 + 8.0)] + [(0.0, 10.0)] * (dim - 1), max_distance=1.0, goal_bias=goal_bias, lvs_fraction=0.05,
                start=[X0 + 1.0] + [1.0] * (dim - 1), goal_centre=[X0 + 7.0] + [9.0] * (dim - 1), goal_radius=0.5, spheres=None,
                boxes=(np.array([[X0 + 3.5] + [-1.0] * (dim - 1)]), np.array([[X0 + 4.5] + [11.0] * (dim - 1)])))


def se2_scene():
    return dict(bounds_xy=[(X0, X0 + 8.0), (0.0, 10.0)], theta_bounds=(-math.pi, math.pi), max_distance=1.0, goal_bias=0.05, lvs_fraction=0.05,
                start=[X0 + 1.0, 1.0, 0.0], goal_centre=[X0 + 7.0, 9.0, 0.0], goal_radius=0.5, clearance=0.25,
                segments=np.array([[X0 + 4.0, -1.0, X0 + 4.0, 11.0]]))


@functools.lru_cache(maxsize=None)
def rejections(bounds, goal_bias, disc, pid, iterations=ITERS):
    """(rejected range draws, per aligned block of 64 iterations) of problem `pid` over its first `iterations` iterations: the
    stream replayed with make_golden's ChaCha12Rng, random_bool and random_range (a call that used n words rejected n - 1)"""
    rng = mg.ChaCha12Rng(SEED, pid)
    per_block = [0] * ((iterations + 63) // 64)
    for it in range(iterations):
        if mg.random_bool(rng, goal_bias):
            if disc:   # sample_goal of the disc fixture: the angle by random_range, then one word for the radius
                before = rng.draws
                mg.random_range(rng, 0.0, 2.0 * math.pi)
                per_block[it // 64] += rng.draws - before - 1
                rng.next_u64()
            continue
        for lo, hi in bounds:
            before = rng.draws
            mg.random_range(rng, lo, hi)
            per_block[it // 64] += rng.draws - before - 1
    return sum(per_block), tuple(per_block)


def assert_every_problem_redraws(bounds, goal_bias=0.05, disc=False, iterations=None):
    """the condition the whole file rests on: every problem has a rejected draw; over the case, blocks with and without one"""
    with_one = without = 0
    for p in range(P):
        total, per_block = rejections(tuple(bounds), goal_bias, disc, p, iterations[p] if iterations else ITERS)
        assert total >= 1, ("no rejected draw in problem", p)
        with_one += sum(1 for b in per_block if b)
        without += sum(1 for b in per_block if not b)
    assert with_one > 0 and without > 0


@functools.lru_cache(maxsize=None)
def rrt_oracles(dim, goal_bias=0.05, disc=False):
    """the oracle's runs of one scene, shared by the kernels compared with them: after ITERS iterations and after MORE further ones"""
    sc = scene(dim, goal_bias)
    out = []
    for iters in (ITERS, ITERS + MORE):
        planners = []
        for p in range(P):
            o = orc.OracleRRT(dim, sc["bounds"], sc["max_distance"], goal_bias, sc["lvs_fraction"], MAX_NODES, False, SEED, p)
            if disc:
                o.set_goal_sampler(1)
            o.set_boxes(*sc["boxes"])
            o.setup(sc["start"], sc["goal_centre"], sc["goal_radius"])
            o.solve(ITERS)
            if iters > ITERS:
                o.solve(iters - ITERS)
            planners.append(o)
        out.append(planners)
    return out


def same_rrt(g, p, o, c):
    assert int(c["nodes"][p]) == o.num_nodes and int(c["iterations"][p]) == o.iterations and int(c["accepted"][p]) == o.accepted
    assert int(c["checksum"][p]) == o.checksum and int(c["goal_node"][p]) == o.goal_node
    assert int(c["stop_reason"][p]) == o.stop_reason == capi.STOP_ITERATIONS
    gs, gp = g.tree(p)
    os_, op = o.tree()
    assert np.array_equal(gp, op) and np.array_equal(bits(gs), bits(os_))


def gpu_rrt(sc, kernel, **extra):
    """every shape of this file has an instantiation of its kernel: a refusal at create is a failure"""
    return scenarios.make_batch(sc, P, MAX_NODES, False, SEED, 0, 0, kernel, **extra)


def run_rrt(dim, kernel, goal_bias=0.05, disc=False, **extra):
    sc = scene(dim, goal_bias)
    assert_every_problem_redraws(sc["bounds"], goal_bias, disc)
    at_iters, at_more = rrt_oracles(dim, goal_bias, disc)
    if disc:
        extra["goal_sampler"] = capi.GOAL_SAMPLE_UNIFORM_DISC
    g = gpu_rrt(sc, kernel, **extra)
    g.solve(ITERS)
    c = g.counts()
    for p in range(P):
        assert at_iters[p].iterations == ITERS and at_iters[p].goal_node < 0   # the wall holds: no solution, every iteration ran
        same_rrt(g, p, at_iters[p], c)
    g.solve(MORE)   # starts at the stream position the first launch left
    c = g.counts()
    for p in range(P):
        same_rrt(g, p, at_more[p], c)
    return g


@pytest.mark.parametrize("dim", [2, 3])
def test_cells_growing(dim):
    run_rrt(dim, capi.KERNEL_CELLS).close()


@pytest.mark.parametrize("dim", [2, 3, 4])
def test_lanes(dim):
    run_rrt(dim, capi.KERNEL_LANES).close()


def test_resident():
    run_rrt(3, capi.KERNEL_RESIDENT).close()


def test_stream_control():
    """the streaming kernel samples one iteration at a time (sample_state): the scene itself agrees with the oracle"""
    run_rrt(7, capi.KERNEL_STREAM).close()


@pytest.mark.parametrize("kernel", [capi.KERNEL_CELLS, capi.KERNEL_LANES], ids=["cells", "lanes"])
def test_disc_goal_sampler(kernel):
    run_rrt(2, kernel, goal_bias=0.3, disc=True).close()


def test_cells_frozen_split_fast_forwards_across_rejected_draws():
    """A frozen launch cut into three parts: the parts behind the first find their start by running the sampler's position
    arithmetic over the iterations in front of them, storing nothing -- across blocks that hold a rejected draw.  The tree is the
    one the growing run left, handed to a fresh batch (set_tree), so the frozen launch starts at the head of the stream and draws
    the very words whose rejections were counted."""
    dim, split, rounds = 3, 3, ITERS // 64
    sc = scene(dim)
    assert_every_problem_redraws(sc["bounds"])
    # Part k starts at round rounds * k / split or later (the later parts get fewer rounds, never more).  So the last part
    # fast-forwards over at least the first rounds * (split - 1) / split rounds, and every later part over the first
    # rounds / split: rejected draws must lie there, not only somewhere in the launch.
    per_block = [rejections(tuple(sc["bounds"]), sc["goal_bias"], False, p)[1] for p in range(P)]
    assert all(any(b[:rounds * (split - 1) // split]) for b in per_block)
    assert any(any(b[:rounds // split]) for b in per_block)
    grown = rrt_oracles(dim)[0]
    g = gpu_rrt(sc, capi.KERNEL_CELLS, frozen_split=split)
    planners = []
    for p in range(P):
        states, parents = grown[p].tree()
        o = orc.OracleRRT(dim, sc["bounds"], sc["max_distance"], sc["goal_bias"], sc["lvs_fraction"], MAX_NODES, False, SEED, p)
        o.set_boxes(*sc["boxes"])
        o.setup(sc["start"], sc["goal_centre"], sc["goal_radius"])
        assert o.set_tree(states, parents) == 0
        g.set_tree(p, states, parents)
        planners.append(o)
    g.solve(ITERS, freeze=True)
    c = g.counts()
    for p, o in enumerate(planners):
        o.solve(ITERS, freeze=True)
        assert int(c["nodes"][p]) == o.num_nodes == grown[p].num_nodes
        same_rrt(g, p, o, c)
    g.solve(MORE)   # growing again, from the stream position the last part left
    c = g.counts()
    for p, o in enumerate(planners):
        o.solve(MORE)
        same_rrt(g, p, o, c)
    g.close()


@pytest.mark.parametrize("dim", [2, 3, 7])
def test_rrt_connect(dim):
    """R^7 samples 32 iterations at a time: 64 x (1 + 7) words do not fit the window's 504 usable words"""
    sc = scene(dim)
    assert_every_problem_redraws(sc["bounds"])
    g = scenarios.make_batch(sc, P, MAX_NODES, True, SEED, 0, 0, 0, capi.PLANNER_RRT_CONNECT)
    planners = []
    for p in range(P):
        o = orc.OracleRRTConnect(dim, sc["bounds"], sc["max_distance"], sc["goal_bias"], sc["lvs_fraction"], MAX_NODES, SEED, p)
        o.set_boxes(*sc["boxes"])
        o.setup(sc["start"], sc["goal_centre"], sc["goal_radius"])
        planners.append(o)
    for iters in (ITERS, MORE):
        g.solve(iters)
        c, gc = g.counts(), g.goal_counts()
        for p, o in enumerate(planners):
            assert o.solve(iters) == orc.NO_SOLUTION_FOUND
            assert int(c["nodes"][p]) == o.num_nodes(0) and int(gc["nodes"][p]) == o.num_nodes(1)
            assert int(c["iterations"][p]) == o.iterations and int(c["checksum"][p]) == o.checksum
            assert int(c["goal_node"][p]) == o.end_node(0) == -1 and int(gc["end_node"][p]) == o.end_node(1)
            assert int(c["stop_reason"][p]) == o.stop_reason == capi.STOP_ITERATIONS
            for which, (gs, gp) in enumerate((g.tree(p), g.goal_tree(p))):
                os_, op = o.tree(which)
                assert np.array_equal(gp, op) and np.array_equal(bits(gs), bits(os_))
        if iters == ITERS:
            assert all(o.iterations == ITERS for o in planners)
    g.close()


def test_se2_rrt_connect():
    """SE(2): the stream of an R^3 problem (one Bernoulli word, then x, y, theta by random_range); a closed wall of segments"""
    sc = se2_scene()
    bounds = list(sc["bounds_xy"]) + [sc["theta_bounds"]]
    g = capi.RRTBatch(3, bounds, sc["max_distance"], sc["goal_bias"], P, MAX_NODES, sc["lvs_fraction"], True, SEED, 0, 0, capi.KERNEL_AUTO,
                      capi.PLANNER_RRT_CONNECT, 0.0, capi.SPACE_SE2)
    g.set_segments(sc["segments"], sc["clearance"])
    g.setup(sc["start"], sc["goal_centre"], sc["goal_radius"])
    planners = []
    for p in range(P):
        o = orc.OracleSE2Connect(sc["bounds_xy"], sc["theta_bounds"], sc["max_distance"], sc["goal_bias"], sc["lvs_fraction"], MAX_NODES, SEED, p)
        o.set_segments(sc["segments"], sc["clearance"])
        o.setup(sc["start"], sc["goal_centre"], sc["goal_radius"])
        planners.append(o)
    for iters in (ITERS, MORE):
        g.solve(iters)
        c, gc = g.counts(), g.goal_counts()
        for p, o in enumerate(planners):
            assert o.solve(iters) == orc.NO_SOLUTION_FOUND
            assert int(c["nodes"][p]) == o.num_nodes(0) and int(gc["nodes"][p]) == o.num_nodes(1)
            assert int(c["iterations"][p]) == o.iterations and int(c["checksum"][p]) == o.checksum
            assert int(c["goal_node"][p]) == o.end_node(0) == -1 and int(gc["end_node"][p]) == o.end_node(1)
            assert int(c["stop_reason"][p]) == o.stop_reason
            for which, (gs, gp) in enumerate((g.tree(p), g.goal_tree(p))):
                os_, op = o.tree(which)
                assert np.array_equal(gp, op) and np.array_equal(bits(gs), bits(os_))
        if iters == ITERS:   # each problem keeps a rejection before its run ends (a run may end early at the node cap)
            assert_every_problem_redraws(bounds, sc["goal_bias"], iterations=[o.iterations for o in planners])
    g.close()
