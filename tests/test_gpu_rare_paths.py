"""-m gpu: the rarely taken paths of the screened kernels, forced one at a time through oxhip_rrt_config.debug_flags and run
over the golden matrix (README scene, the reference's wall scene, configs[1] batch), in the product instantiation AND in the
stamped one whose counters prove the path was really taken.  The golden scenes run rrt_lanes.hip (the lane-per-query kernel);
the configs[1] batch runs it and rrt_cells.hip (the cell-grid kernel, what KERNEL_AUTO runs in R^2 / R^3), which honours
DEBUG_ALL_WHOLE_TREE and DEBUG_ONE_LANE_ROUNDS and ignores the other two switches (it has no pair pass, and its memo lasts
while the tree has not grown).

  DEBUG_ALL_WHOLE_TREE    no screen verdict is trusted: every query takes the whole-tree path (one query at a time, the wave
                          scanning the binary64 tree) unless the memoized whole-tree answer applies (the
                          memo holds the LAST whole-tree query: with goal_bias 0.5 a goal-centre query follows another one a
                          quarter of the time -- test_goal_bias_half_memo_is_reused_and_refreshed)
  DEBUG_SHORT_MEMO        ... and the memo expires after 8 inserts, so it is refreshed (whole-tree path) and reused in turns
  DEBUG_ONE_LANE_ROUNDS   a round commits one lane: every other lane is re-resolved against the grown tree (the ring fold picks
                          the new nodes up), i.e. a conflict cut every round
  DEBUG_PAIR_TO_WHOLE_TREE two-lane near-ties take the whole-tree path (the product resolves them in the round)
  (rrt_lanes.hip: the committed-node ring wraps in every tree beyond 256 nodes: counted, asserted on the configs[1] batch)

VERDICT round 2, weak item 2: a wrong accept in the whole-tree path reached the default kernel with 165 tests green.
Reference semantics at stake: the strict '<' / lowest-index argmin of rrt.rs:187-196 and check_motion rrt.rs:90-116."""
import os
import subprocess
import sys
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oxmpl_amd import capi, scenarios  # noqa: E402
from oracle import oracle_py as orc  # noqa: E402
from helpers import bits, hexf, params_boxes, params_spheres  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# stamp words (include/oxmpl_hip.h): batch-wide sums
W_WHOLE_TREE, W_MEMO, W_CONFLICT, W_RING_WRAP, W_PAIR, W_FORCED_CUT = 54, 55, 56, 57, 58, 59

FLAGS = {
    "all_whole_tree": capi.DEBUG_ALL_WHOLE_TREE,
    "all_whole_tree_short_memo": capi.DEBUG_ALL_WHOLE_TREE | capi.DEBUG_SHORT_MEMO,
    "one_lane_rounds": capi.DEBUG_ONE_LANE_ROUNDS,
    "pair_to_whole_tree": capi.DEBUG_PAIR_TO_WHOLE_TREE,
    "one_lane_rounds_and_whole_tree": capi.DEBUG_ONE_LANE_ROUNDS | capi.DEBUG_ALL_WHOLE_TREE,
}


def _oracle(sc, seed, pid, max_nodes, stop):
    o = orc.OracleRRT(sc["dim"], sc["bounds"], sc["max_distance"], sc["goal_bias"], sc["lvs_fraction"], max_nodes, stop, seed, pid)
    if sc["spheres"] is not None:
        o.set_spheres(*sc["spheres"])
    if sc["boxes"] is not None:
        o.set_boxes(*sc["boxes"])
    o.setup(sc["start"], sc["goal_centre"], sc["goal_radius"])
    return o


def _same(gpu, p, o, c):
    assert int(c["nodes"][p]) == o.num_nodes and int(c["iterations"][p]) == o.iterations
    assert int(c["accepted"][p]) == o.accepted and int(c["checksum"][p]) == o.checksum
    assert int(c["goal_node"][p]) == o.goal_node
    gs, gp = gpu.tree(p)
    os_, op = o.tree()
    assert np.array_equal(gp, op) and np.array_equal(bits(gs), bits(os_))
    assert np.array_equal(bits(gpu.path(p)), bits(o.path()))


def _check_counters(name, s, iterations):
    if "whole_tree" in name and "pair" not in name:
        assert int(s[W_WHOLE_TREE]) + int(s[W_MEMO]) >= 0.95 * iterations, (int(s[W_WHOLE_TREE]), int(s[W_MEMO]), iterations)
        assert int(s[W_WHOLE_TREE]) > 0
    if "one_lane" in name and "whole_tree" not in name:   # (with no verdict trusted a round never gets past its first lane anyway)
        assert int(s[W_FORCED_CUT]) > 0


@pytest.mark.parametrize("stamped", [False, True], ids=["product_build", "stamped_build"])
@pytest.mark.parametrize("name", list(FLAGS))
@pytest.mark.parametrize("key", ["config1", "wall"])
def test_golden_fixtures_under_forced_paths(golden, key, name, stamped):
    params = golden[key]["params"]
    sc = dict(dim=params["dim"], bounds=params["bounds"], max_distance=params["max_distance"], goal_bias=params["goal_bias"],
              lvs_fraction=params["fraction"], start=params["start"], goal_centre=params["goal_c"], goal_radius=params["goal_r"],
              spheres=params_spheres(params) if params["spheres"] else None, boxes=params_boxes(params) if params["boxes"] else None)
    for run in golden[key]["runs"]:
        gpu = scenarios.make_batch(sc, 1, 10000, True, run["seed"], run["pid"], 0, capi.KERNEL_LANES, debug_flags=FLAGS[name])
        if stamped:
            gpu.enable_stamps(True)
        st = gpu.solve(params["max_iterations"])
        assert st[0] == capi.OK
        c = gpu.counts()
        assert int(c["nodes"][0]) == run["n"] and int(c["iterations"][0]) == run["iterations"]
        assert "%016x" % int(c["checksum"][0]) == run["checksum"] and int(c["goal_node"][0]) == run["goal_node"]
        states, parents = gpu.tree(0)
        m = len(run["first_parents"])
        assert [[hexf(v) for v in row] for row in states[:m]] == run["first_states"]
        assert list(parents[:m]) == run["first_parents"]
        assert [[hexf(v) for v in row] for row in gpu.path(0)] == run["path"]
        if stamped:
            _check_counters(name, gpu.stamps(), run["iterations"])
        gpu.close()


@pytest.mark.parametrize("stamped", [False, True], ids=["product_build", "stamped_build"])
@pytest.mark.parametrize("name", list(FLAGS) + ["none"])
def test_config2_batch_under_forced_paths(name, stamped):
    """configs[1]'s scene, 12 problems x 1,500 growing + 300 frozen iterations (resume in between), against the oracle"""
    _config2_batch_under_forced_paths(capi.KERNEL_LANES, name, stamped)


@pytest.mark.parametrize("stamped", [False, True], ids=["product_build", "stamped_build"])
@pytest.mark.parametrize("name", list(FLAGS) + ["none"])
def test_config2_batch_under_forced_paths_cells(name, stamped):
    """the same batch on the cell-grid kernel: its whole-tree ([54] / [55]), forced-cut ([59]) and conflict-cut ([56]) counters"""
    _config2_batch_under_forced_paths(capi.KERNEL_CELLS, name, stamped)


def _config2_batch_under_forced_paths(kernel, name, stamped):
    sc = scenarios.config2()
    P, grow, frozen = 12, 1500, 300
    flags = FLAGS.get(name, 0)
    gpu = scenarios.make_batch(sc, P, 10000, False, 42, 0, 0, kernel, debug_flags=flags)
    if stamped:
        gpu.enable_stamps(True)
    gpu.solve(700)
    gpu.solve(grow - 700)
    assert gpu.last_timing()["kernel"] == kernel
    s_grow = gpu.stamps() if stamped else None
    gpu.solve(frozen, freeze=True)
    planners = [_oracle(sc, 42, p, 10000, False) for p in range(P)]
    orc.solve_many(planners, grow, threads=6)
    orc.solve_many(planners, frozen, freeze=True, threads=6)
    c = gpu.counts()
    for p in range(P):
        _same(gpu, p, planners[p], c)
    if stamped:
        _check_counters(name, s_grow, P * grow)               # (the batch-wide counters add up over the launches)
        if kernel == capi.KERNEL_LANES:
            assert int(s_grow[W_RING_WRAP]) >= P              # every tree passed a multiple of the ring size
        if name == "none":
            # the product's own behaviour on this scene: conflict cuts happen (a growing tree), the whole-tree path is rare
            assert int(s_grow[W_CONFLICT]) > 0
            assert int(s_grow[W_WHOLE_TREE]) < 0.05 * P * grow
    gpu.close()


def test_goal_bias_half_memo_is_reused_and_refreshed():
    """goal_bias 0.5: half of all queries are the goal centre; with no screen verdict trusted they are answered from the memoized
    whole-tree answer, which the short expiry forces to be rebuilt over and over"""
    sc = dict(scenarios.config2(), goal_bias=0.5)
    P, iters = 6, 1200
    for flags in (capi.DEBUG_ALL_WHOLE_TREE, capi.DEBUG_ALL_WHOLE_TREE | capi.DEBUG_SHORT_MEMO):
        gpu = scenarios.make_batch(sc, P, 4000, False, 9, 300, 0, capi.KERNEL_LANES, debug_flags=flags)
        gpu.enable_stamps(True)
        gpu.solve(iters)
        s = gpu.stamps()
        planners = [_oracle(sc, 9, 300 + p, 4000, False) for p in range(P)]
        orc.solve_many(planners, iters, threads=6)
        c = gpu.counts()
        for p in range(P):
            _same(gpu, p, planners[p], c)
        assert int(s[W_MEMO]) > (0.03 if flags & capi.DEBUG_SHORT_MEMO else 0.1) * P * iters, int(s[W_MEMO])
        gpu.close()


def test_rank7_shard_of_configs2():
    """BASELINE.json configs[2]: rank 7 of 8 owns the global problem ids 7168 .. 8191 (the id is the ChaCha stream id): 24 of them,
    600 iterations, against the oracle's problems with the same ids"""
    sc = scenarios.config2()
    first = 7 * 1024
    for kernel in (capi.KERNEL_AUTO, capi.KERNEL_STREAM):
        gpu = scenarios.make_batch(sc, 24, 10000, False, 42, first, 0, kernel)
        gpu.solve(600)
        planners = [_oracle(sc, 42, first + p, 10000, False) for p in range(24)]
        orc.solve_many(planners, 600, threads=8)
        c = gpu.counts()
        for p in range(24):
            _same(gpu, p, planners[p], c)
        gpu.close()


def test_bench_py_n2_branch_runs_with_two_ranks_on_one_gpu(tmp_path):
    """bench.py's N > 1 branch, executed: two ranks (torch.distributed.run, gloo for the barriers and the one all-gather -- both ranks
    share GPU 0, which RCCL refuses), each rank its own shard of problem ids, each checking two of its problems against the oracle
    (--full) before rank 0 prints.  A functional run, not a scaling point."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--problems", "64", "--iters", "512", "--backend", "gloo", "--device-map", "0,0", "--full"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["n_gpus"] == 2 and out["scaling"] == "weak"
    pr = out["per_rank"]
    assert pr["first_problem_id"] == [0, 64] and pr["device"] == [0, 0]
    assert pr["problems_checked_against_oracle"] == [2, 2]
    assert len(pr["iterations_per_s"]) == 2 and min(pr["iterations_per_s"]) > 0
    assert abs(out["value"] - 2 * 64 * 512 * 2 / (out["ms_per_step"] * 2 * 1e-3)) / out["value"] < 1e-6
    assert "cpu_baseline" not in out   # rank 0 at N = 1 only
