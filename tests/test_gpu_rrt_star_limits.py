"""-m gpu: RRT* at its limits, against the CPU oracle (orc_rrts_*) bit for bit through test_gpu_rrt_star.py's assert_same contract
(nodes, iterations, accepted, checksum, goal node, tree bits, parents after rewiring, cost bits, path bits) -- no tolerance anywhere.
The scenes are tests/rrt_star_limits_shapes.py; that each holds what its test here relies on (counted by an instrumented replay that
agrees with the oracle bit for bit) is held on the CPU by tests/test_rrt_star_limits_model.py.  Every case runs on KERNEL_CELLS where
cells_supported holds (R^2, R^3), on KERNEL_LANES where lanes_supported holds (R^2 .. R^6) -- both wired by rrt_star_wire.hip -- and
on KERNEL_STREAM (rrt_star.hip).
  slab    star_shadow / star_pairs / star_edges <4..6> by name; hundreds of rewires, changed parents and refused neighbour motions in
          every dimension: step 8 of star_wire and the `ba` flag; spheres 65 .. 100 (the chunk of star_edges that never has a mask
          grid) next to a box
  reach   thousands of exact cost ties: the strict < against the nearest node's route, the lowest index among equal minima, strictness
          between the 64-entry blocks of a list, the strict < of rewiring; also on the two-pass / one-segment path and with the
          pool cut to its minimum
  R^1, R^7, R^8   KERNEL_AUTO resolves to the one-kernel design; the decoupled designs are refused
  mixed   problems of one batch that end at 2 nodes, at a bit-equal copy of the goal, or at the node cap; one neighbour entry next
          to a round of 130,000 in eight segments
  frames  the R^5 slab far from the origin, at 1e40 (no binary32 screen) and at 1e-12
  large   33,000 nodes: node indices beyond 2^15 in star_pairs' 16-bit hit buffer and rrt_cells.hip's 16-bit node names"""
import numpy as np
import pytest

import rrt_star_limits_shapes as shapes
from helpers import bits, params_boxes, params_spheres
from oxmpl_amd import capi

pytestmark = pytest.mark.gpu

KERNELS = {"cells": capi.KERNEL_CELLS, "lanes": capi.KERNEL_LANES, "stream": capi.KERNEL_STREAM}
CUTS = (90, 160)                 # the budgets of the first two of three solve calls
TWO_PASS_ONE_SEGMENT = capi.DEBUG_STAR_TWO_PASS | capi.DEBUG_STAR_ONE_SEGMENT


def designs(dim):
    return (["cells"] if dim in (2, 3) else []) + (["lanes"] if 2 <= dim <= 6 else []) + ["stream"]


DIM_DESIGN = [pytest.param(dim, d, id="R%d-%s" % (dim, d)) for dim in range(2, 7) for d in designs(dim)]
# how a case is run: (solve budgets, debug flags, star_pool_share); the last two belong to the decoupled design
RUNS = {"one_call": ((shapes.BUDGET,), 0, 0), "three_calls": (CUTS + (shapes.BUDGET,), 0, 0),
        "two_pass_one_segment": ((shapes.BUDGET,), TWO_PASS_ONE_SEGMENT, 0), "pool_share_1": ((shapes.BUDGET,), 0, 1)}
REACH_CASES = [pytest.param(p.values[0], p.values[1], run, id="%s-%s" % (p.id, run)) for p in DIM_DESIGN for run in RUNS
               if p.values[1] != "stream" or run in ("one_call", "three_calls")]


def make_gpu(P, design, n_problems, seed, first_pid, stop=False, **extra):
    kernel = KERNELS[design] if design in KERNELS else design
    g = capi.RRTBatch(P["dim"], P["bounds"], P["max_distance"], P["goal_bias"], n_problems, P["max_nodes"], P["fraction"], stop, seed,
                      first_pid, 0, kernel, capi.PLANNER_RRT_STAR, P["search_radius"], **extra)
    if P["spheres"]:
        g.set_spheres(*params_spheres(P))
    if P["boxes"]:
        g.set_boxes(*params_boxes(P))
    g.setup(P["start"], P["goal_c"], P["goal_r"])
    return g


def assert_same(g, p, o, c=None):
    """test_gpu_rrt_star.py's contract, restated (importing that module would bring its autouse fixture along)"""
    c = c or g.counts()
    assert int(c["nodes"][p]) == o.num_nodes
    assert int(c["iterations"][p]) == o.iterations
    assert int(c["accepted"][p]) == o.accepted
    assert int(c["checksum"][p]) == o.checksum
    assert int(c["goal_node"][p]) == o.goal_node
    gs, gp = g.tree(p)
    os_, op = o.tree()
    assert np.array_equal(bits(gs), bits(os_)) and np.array_equal(gp, op)
    assert np.array_equal(bits(g.costs(p)), bits(o.costs()))
    gpath, opath = g.path(p), o.path()
    assert gpath.shape == opath.shape and np.array_equal(bits(gpath), bits(opath))


def assert_kernel(g, design):
    assert g.last_timing()["kernel"] == KERNELS[design]


def run_and_compare(P, design, oracles, seed=shapes.SEED, first_pid=shapes.PIDS[0], run="one_call"):
    budgets, flags, share = RUNS[run]
    g = make_gpu(P, design, len(oracles), seed, first_pid, debug_flags=flags, star_pool_share=share)
    for budget in budgets:
        g.solve(budget)
    assert_kernel(g, design)
    c = g.counts()
    for p, o in enumerate(oracles):
        assert o.num_nodes == P["max_nodes"] and int(c["stop_reason"][p]) == capi.STOP_NODES, p
        assert_same(g, p, o, c)
    g.close()


# ------------------------------------------------------------------------------------------------------- slab and reach, R^2 .. R^6
@pytest.mark.parametrize("run", ["one_call", "three_calls"])
@pytest.mark.parametrize("dim,design", DIM_DESIGN)
def test_slab_scenes(dim, design, run):
    run_and_compare(shapes.slab_scene(dim), design, [shapes.slab_oracle(dim, pid) for pid in shapes.PIDS], run=run)


@pytest.mark.parametrize("variant", shapes.REACH_VARIANTS)
@pytest.mark.parametrize("dim,design,run", REACH_CASES)
def test_reach_scenes(dim, design, run, variant):
    run_and_compare(shapes.reach_scene(dim, variant), design, [shapes.reach_oracle(dim, variant, pid) for pid in shapes.PIDS], run=run)


# ------------------------------------------------------------------------------------------------------- R^1, R^7, R^8
def _scenes_of(dim):
    yield "slab", shapes.slab_scene(dim), [shapes.slab_oracle(dim, pid) for pid in shapes.PIDS]
    for variant in shapes.REACH_VARIANTS:
        yield "reach " + variant, shapes.reach_scene(dim, variant), [shapes.reach_oracle(dim, variant, pid) for pid in shapes.PIDS]


@pytest.mark.parametrize("dim", [1, 7, 8])
def test_dimensions_of_the_one_kernel_design_alone(dim):
    assert designs(dim) == ["stream"]
    for name, P, oracles in _scenes_of(dim):
        g = make_gpu(P, capi.KERNEL_AUTO, len(oracles), shapes.SEED, shapes.PIDS[0])
        g.solve(shapes.BUDGET)
        assert g.last_timing()["kernel"] == capi.KERNEL_STREAM, name      # star_wire_supported covers 2 .. 6
        c = g.counts()
        for p, o in enumerate(oracles):
            assert o.num_nodes == P["max_nodes"], name
            assert_same(g, p, o, c)
        g.close()
    P = shapes.slab_scene(dim)
    for design in ("lanes", "cells"):
        with pytest.raises(capi.OxhipError) as ei:
            make_gpu(P, design, 1, shapes.SEED, shapes.PIDS[0])
        assert ei.value.status == capi.ERR_BAD_ARG, design


# ------------------------------------------------------------------------------------------------------- mixed batch
MIXED = [pytest.param(dim, d, id="R%d-%s" % (dim, d)) for dim in (3, 5) for d in designs(dim)]


@pytest.mark.parametrize("run", sorted(shapes.MIXED_RUNS))
@pytest.mark.parametrize("dim,design", MIXED)
def test_mixed_batch(dim, design, run):
    """every problem against its own oracle after every solve call; wire_new_nodes sizes its launches, and decides between the chunk
    path and the second search and between one segment and eight, by the whole batch"""
    P = shapes.mixed_scene(dim, run)
    n_prob = len(shapes.MIXED_RADII)
    g = make_gpu(P, design, n_prob, shapes.SEED, shapes.PIDS[0], stop=True)
    done, ends = 0, set()
    for budget in shapes.MIXED_RUNS[run][1]:
        st = g.solve(budget)
        done += budget
        c = g.counts()
        for p in range(n_prob):
            o = shapes.mixed_oracle(dim, run, p, done)
            assert_same(g, p, o, c)
            assert (int(st[p]) == capi.OK) == (o.goal_node >= 0), p
            assert int(st[p]) in (capi.OK, capi.ERR_NO_SOLUTION_FOUND), p
            ends.add((o.num_nodes, int(c["stop_reason"][p])))
    assert_kernel(g, design)
    assert (2, capi.STOP_GOAL) in ends and (P["max_nodes"], capi.STOP_NODES) in ends
    g.close()


# ------------------------------------------------------------------------------------------------------- frames
@pytest.mark.parametrize("design", designs(shapes.FRAME_DIM))
@pytest.mark.parametrize("frame", sorted(shapes.FRAMES))
def test_frames(frame, design):
    oracles = [shapes.frame_oracle(frame, pid) for pid in shapes.FRAME_PIDS]
    run_and_compare(shapes.frame_scene(frame), design, oracles)


# ------------------------------------------------------------------------------------------------------- large tree
@pytest.mark.parametrize("design", ["auto", "stream"])
def test_large_tree(design):
    P, o = shapes.large_scene(), shapes.large_oracle()
    _, parents = o.tree()
    assert int((parents >= shapes.HALF_U16).sum()) >= 100
    g = make_gpu(P, capi.KERNEL_AUTO if design == "auto" else design, 1, shapes.LARGE_SEED, shapes.LARGE_PID)
    g.solve(shapes.BUDGET)
    assert g.last_timing()["kernel"] == (capi.KERNEL_CELLS if design == "auto" else capi.KERNEL_STREAM)   # AUTO: the cells geometry
    assert_same(g, 0, o)
    g.close()


def test_large_tree_is_beyond_the_lanes_kernel():
    """lanes_supported: 20,480 nodes at most in R^2 (40 rows of 512); alloc_star refuses the design rather than changing it"""
    with pytest.raises(capi.OxhipError) as ei:
        make_gpu(shapes.large_scene(), "lanes", 1, shapes.LARGE_SEED, shapes.LARGE_PID)
    assert ei.value.status == capi.ERR_BAD_ARG
