"""-m gpu: RRTConnect over SE(3) (OXHIP_SPACE_SE3, rrt_connect_se3.hip) against the CPU checker (tests/golden/make_golden_se3.py)
and its golden file, bit for bit -- no tolerance anywhere: the kernel and the checker are the same unfused binary64 operations.
The SE(3) arithmetic (distance, interpolate, rot), the rigid-body validity check, both trees, parents, counters, checksums, end
nodes and merged paths; the field scene x 1024 and the slot scene x 256 against the recorded counts, every problem solved; batch
sizes, launch cuts, resumed solves, stream shifts, stop reasons, a translated frame, a fuzz leg and the Python surface.
PARITY UNPINNED against oxmpl itself (the space does not exist there)."""
import json
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import make_golden as mg  # noqa: E402
import make_golden_se3 as se3  # noqa: E402
import make_golden_so3 as so3  # noqa: E402
from helpers import bits, unhex  # noqa: E402
from se3_helpers import assert_same, config_bounds, make_gpu, rows as _rows  # noqa: E402
from oxmpl_amd import capi, scenarios  # noqa: E402

BUDGET = 20000


@pytest.fixture(scope="module")
def se3_golden():
    with open(os.path.join(ROOT, "tests", "golden", "se3_golden.json")) as f:
        return json.load(f)


def scene(golden, name):
    return se3.scene_from_params(golden[name]["params"], golden)


def from_record(rec):
    """a golden run -> the shape of a checker result"""
    states = [[[unhex(v) for v in row] for row in t] for t in rec["states"]]
    return dict(n=rec["n"], iterations=rec["iterations"], checksum=int(rec["checksum"], 16), end=rec["end"], states=states,
                parents=rec["parents"], path=[states[w][i] for w, i in rec["path_nodes"]])


def assert_path_ok(path, sc, body):
    """the reference's path assertions (rrt_connect_so3ss_tests.rs): starts at the start, ends in the goal, valid throughout"""
    path = [list(map(float, row)) for row in path]
    assert len(path) >= 2
    assert np.array_equal(bits(path[0]), bits(sc["start"]))
    assert se3.distance(path[-1], sc["target"]) <= sc["goal_r"]
    assert se3.is_path_valid(path, body, sc["bounds_xyz"], sc["fraction"])


# ------------------------------------------------------------------------------------------------------------ arithmetic
def _unit(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _pairs_at(rng, n, cosines):
    """pairs (a, b) of unit quaternions with dot(a, b) ~ the given cosines (b = cos a + sin u, u orthogonal to a)"""
    a = _unit(rng, n)
    u = rng.normal(size=(n, 4))
    u -= (u * a).sum(axis=1, keepdims=True) * a
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    c = np.asarray(cosines, dtype=np.float64).reshape(-1, 1)
    return a, c * a + np.sqrt(np.maximum(0.0, 1.0 - c * c)) * u


def test_se3_ops_bitwise():
    rng = np.random.default_rng(16)
    n = 12000
    cos = np.concatenate([rng.uniform(-1.0, 1.0, 6000), 0.9995 + rng.uniform(-1e-6, 1e-6, 1500), -0.9995 + rng.uniform(-1e-6, 1e-6, 500),
                          (1.0 - 1e-9) + rng.uniform(-2e-10, 2e-10, 1500), np.full(500, -1.0), np.full(500, 1.0),
                          rng.uniform(-1e-9, 1e-9, 1500)])
    qa, qb = _pairs_at(rng, n, cos)
    qb[6500:7000] = -qa[6500:7000]                       # antipodal quaternions: the same rotation
    pa = rng.uniform(-10.0, 10.0, (n, 3))
    pb = rng.uniform(-10.0, 10.0, (n, 3))
    pb[:400] = pa[:400]                                  # equal positions
    pa[400:800] += 1e6
    pb[400:800] += 1e6                                   # positions at 1e6
    pa[800:1200] *= 1e-13
    pb[800:1200] *= 1e-13                                # ... and at 1e-12
    pa[1200:1400] = pb[1200:1400] = 0.0
    t = rng.uniform(0.0, 1.0, n)
    t[::7] = 0.0
    t[3::7] = 1.0
    a, b = np.hstack([pa, qa]), np.hstack([pb, qb])
    d = capi.se3_op_batch(0, a, b)
    it = capi.se3_op_batch(1, a, b, t)
    v = rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-3.0, 3.0, (n, 1))
    bv = np.hstack([v, np.zeros((n, 4))])
    r = capi.se3_op_batch(2, a, bv)
    assert d.shape == (n,) and it.shape == (n, 7) and r.shape == (n, 3)
    for i in range(n):
        ai, bi = a[i].tolist(), b[i].tolist()
        assert bits(d[i]) == bits(se3.distance(ai, bi)), i
        assert np.array_equal(bits(it[i]), bits(se3.interpolate(ai, bi, float(t[i])))), i
        assert np.array_equal(bits(r[i]), bits(se3.body_centre(ai, v[i].tolist()))), i


def _b16():
    return [([-1.2 + 0.16 * i, 0.05 * (i % 3), -0.04 * (i % 4)], 0.1 + 0.01 * i) for i in range(16)]


def test_validity_and_motions_bitwise(se3_golden):
    fld, slt = scene(se3_golden, "field"), scene(se3_golden, "slot")
    start3, target3 = fld["start"][:3], fld["target"][:3]
    n_lds = 128   # obstacles the kernel stages in LDS: one more takes the instantiation that reads them from HBM
    fields = {0: [], 1: fld["obstacles"][:1], 64: fld["obstacles"], 110: slt["obstacles"],
              n_lds + 1: se3.field_spheres(0x5EED0017, n_lds + 1, -4.5, 4.5, 0.2, 0.6, [start3, target3], 1.6)}
    bodies = {1: [([0.0, 0.0, 0.0], 0.0)], 5: se3.ROD, 16: _b16()}
    rng = mg.ChaCha12Rng(99, 1)
    seen = set()
    for n_obs, obstacles in fields.items():
        for n_body, body in bodies.items():
            sc = dict(fld, obstacles=obstacles, body=body)
            chk = se3.make_body(sc)
            g = make_gpu(sc, 1, 0, 0)
            states = [se3.sample_uniform(rng, sc["bounds_xyz"], [0.0, 0.0, 0.0, 1.0], se3.PI) for _ in range(160)]
            if n_obs == 110:   # near the slot's plane, where the orientation decides
                for s in states[:80]:
                    s[0], s[2] = s[0] * 0.2, s[2] * 0.05
            want = [chk.is_valid(s) for s in states]
            assert g.is_valid(np.array(states)).tolist() == want, (n_obs, n_body)
            frm, to = [], []
            for i in range(120):
                a = states[i]
                q = se3.sample_uniform(rng, sc["bounds_xyz"], [0.0, 0.0, 0.0, 1.0], se3.PI)
                d = se3.distance(a, q)
                step = (0.05, 0.3, 1.0, 2.5)[i % 4]          # one state; a few; the planner's; two dozen
                frm.append(a)
                to.append(se3.interpolate(a, q, step / d) if d > step else q)
            frm.append(states[0])
            to.append(states[0])                                 # a motion of length 0
            wantm = [se3.check_motion(chk, sc["bounds_xyz"], sc["fraction"], a, b) for a, b in zip(frm, to)]
            assert g.check_motion(np.array(frm), np.array(to)).tolist() == wantm, (n_obs, n_body)
            seen.update(want)
            seen.update(wantm)
            g.close()
    assert seen == {True, False}


# ------------------------------------------------------------------------------------------------------------ golden runs
GOLDEN_SCENES = ("field", "slot", "bias1", "point", "bounded", "b16", "n0", "tiny")


@pytest.mark.parametrize("name", GOLDEN_SCENES)
def test_golden_runs(se3_golden, name):
    sc = scene(se3_golden, name)
    for rec in se3_golden[name]["runs"]:
        g = make_gpu(sc, 1, rec["seed"], rec["pid"])
        g.solve(sc["max_iterations"])
        assert_same(g, 0, from_record(rec))
        assert int(g.counts()["stop_reason"][0]) == (capi.STOP_GOAL if rec["end"][0] >= 0 else capi.STOP_ITERATIONS)
        g.close()


@pytest.mark.parametrize("name,count,live", [("field", 1024, 32), ("slot", 256, 4)])
def test_scene_batches_match_the_recorded_counts(se3_golden, name, count, live):
    sc = scene(se3_golden, name)
    rows = se3.count_rows(se3_golden[name])
    assert len(rows) == count
    g = make_gpu(sc, count, se3_golden[name]["count_seed"], 0)
    st = g.solve(BUDGET)
    assert (st == capi.OK).all()                                 # every problem is solved within the budget
    c, gc = g.counts(), g.goal_counts()
    assert (c["stop_reason"] == capi.STOP_GOAL).all() and (c["goal_node"] >= 0).all()
    for p, (its, na, nb, chk) in enumerate(rows):
        assert (int(c["iterations"][p]), int(c["nodes"][p]), int(gc["nodes"][p])) == (its, na, nb), p
        assert int(c["checksum"][p]) == int(chk, 16), p
    body = se3.make_body(sc)
    for p in range(count):
        assert_path_ok(g.path(p), sc, body)
    # against the live checker in full: the first field problems / the slot problems with the fewest recorded iterations
    picks = list(range(live)) if name == "field" else sorted(range(count), key=lambda i: (rows[i][0], i))[:live]
    for p in picks:
        assert_same(g, p, se3.run_scene(sc, se3_golden[name]["count_seed"], p, body=body), c, gc)
    g.close()


# ------------------------------------------------------------------------------------------------------------ batch shapes
def test_problem_0_alone_in_a_batch_cut_and_resumed(se3_golden):
    sc = scene(se3_golden, "field")
    res = se3.run_scene(sc, 42, 0)
    assert res["end"][0] >= 0
    g = make_gpu(sc, 1, 42, 0)
    g.solve(BUDGET)
    assert_same(g, 0, res)
    g.close()
    g = make_gpu(sc, 1024, 42, 0)
    g.solve(BUDGET)
    assert_same(g, 0, res)
    g.close()
    for cut in (1, 7, 64):                                       # launch cuts: the state array carries a problem from launch to launch
        g = make_gpu(sc, 2, 42, 0)
        for _ in range((res["iterations"] + cut - 1) // cut + 2):
            g.solve(cut)
        assert_same(g, 0, res)
        g.close()
    g = make_gpu(sc, 1, 42, 0)                                   # resumed solve calls of uneven length, compared on the way
    done = 0
    for step in (5, 1, 30, 11, BUDGET):
        g.solve(step)
        done = min(done + step, res["iterations"])
        part = se3.run_scene(sc, 42, 0, max_iterations=done)
        assert_same(g, 0, part)
    assert_same(g, 0, res)
    g.close()


def test_first_problem_id_shifts_the_streams(se3_golden):
    sc = scene(se3_golden, "slot")
    rows = se3.count_rows(se3_golden["slot"])
    g = make_gpu(sc, 8, 42, 100)
    g.solve(BUDGET)
    c, gc = g.counts(), g.goal_counts()
    for p in range(8):
        its, na, nb, chk = rows[100 + p]
        assert (int(c["iterations"][p]), int(c["nodes"][p]), int(gc["nodes"][p]), int(c["checksum"][p])) == (its, na, nb, int(chk, 16))
    g.close()


def test_node_cap_and_iteration_budget_stop_reasons(se3_golden):
    sc = scene(se3_golden, "slot")
    body = se3.make_body(sc)
    g = make_gpu(sc, 4, 3, 0, max_nodes=20)                      # the cap on either tree, looked at before any draw
    st = g.solve(BUDGET)
    c = g.counts()
    for p in range(4):
        res = se3.run_scene(sc, 3, p, max_nodes=20, body=body)
        assert res["end"][0] < 0 and max(res["n"]) == 20
        assert_same(g, p, res)
        assert int(c["stop_reason"][p]) == capi.STOP_NODES and int(st[p]) == capi.ERR_NO_SOLUTION_FOUND
    g.solve(50)                                                  # a full tree stays full: nothing moves, no word is drawn
    for p in range(4):
        assert_same(g, p, se3.run_scene(sc, 3, p, max_nodes=20, body=body))
    g.close()
    g = make_gpu(sc, 4, 3, 0)
    st = g.solve(10)
    c = g.counts()
    for p in range(4):
        res = se3.run_scene(sc, 3, p, max_iterations=10, body=body)
        assert res["end"][0] < 0 and res["iterations"] == 10
        assert_same(g, p, res)
        assert int(c["stop_reason"][p]) == capi.STOP_ITERATIONS and int(st[p]) == capi.ERR_NO_SOLUTION_FOUND
    g.close()


def test_translated_frame(se3_golden):
    off = (1.0e6, -5.0e4, 3.0e3)
    for name, pids in (("field", (0, 1, 2, 3)), ("slot", (65, 153))):
        sc = scene(se3_golden, name)
        mv = lambda p: [p[k] + off[k] for k in range(3)]  # noqa: E731
        tr = dict(sc, bounds_xyz=[(lo + off[k], hi + off[k]) for k, (lo, hi) in enumerate(sc["bounds_xyz"])],
                  start=mv(sc["start"]) + sc["start"][3:], target=mv(sc["target"]) + sc["target"][3:],
                  obstacles=[(mv(c), r) for c, r in sc["obstacles"]])
        body = se3.make_body(tr)
        for pid in pids:
            res = se3.run_scene(tr, 42, pid, body=body)
            g = make_gpu(tr, 1, 42, pid)
            st = g.solve(BUDGET)
            assert int(st[0]) == capi.OK and res["end"][0] >= 0   # solved in that frame too
            assert_same(g, 0, res)
            assert_path_ok(g.path(0), tr, body)
            g.close()


def test_fuzz_against_the_checker():
    rng = np.random.default_rng(20261016)
    for case in range(30):
        n_body, n_obs = int(rng.integers(1, 17)), int(rng.choice([0, 1, 3, 17, 64, 110, 128, 129, 140]))
        body = [(rng.uniform(-1.0, 1.0, 3).tolist(), float(rng.choice([0.0, rng.uniform(0.0, 0.4)]))) for _ in range(n_body)]
        obstacles = [(rng.uniform(-5.0, 5.0, 3).tolist(), float(rng.uniform(0.1, 0.8))) for _ in range(n_obs)]
        rot_bounds = None
        if case % 3 == 1:
            rot_bounds = (so3.normalise(rng.normal(size=4).tolist()), float(rng.uniform(0.3, 3.5)))
        lo = rng.uniform(-6.0, -3.0, 3)
        hi = rng.uniform(3.0, 6.0, 3)
        sc = dict(bounds_xyz=[(float(a), float(b)) for a, b in zip(lo, hi)], rot_bounds=rot_bounds,
                  max_distance=float(10.0 ** rng.uniform(-1.3, 0.4)), goal_bias=float(rng.choice([0.0, 0.05, 0.3, 1.0, rng.uniform()])),
                  fraction=float(10.0 ** rng.uniform(-2.0, -0.7)), goal_r=float(rng.uniform(0.05, 0.6)), body=body, obstacles=obstacles,
                  start=rng.uniform(-3.0, 3.0, 3).tolist() + so3.normalise(rng.normal(size=4).tolist()),
                  target=rng.uniform(-3.0, 3.0, 3).tolist() + so3.normalise(rng.normal(size=4).tolist()),
                  max_nodes=int(rng.choice([40, 300, 10000])), max_iterations=int(rng.integers(20, 201)))
        seed, pid = int(rng.integers(0, 1 << 30)), int(rng.integers(0, 1000))
        chk = se3.make_body(sc)
        g = make_gpu(sc, 2, seed, pid)
        g.solve(sc["max_iterations"])
        for p in range(2):
            assert_same(g, p, se3.run_scene(sc, seed, pid + p, body=chk))
        g.close()


def test_python_surface_end_to_end(se3_golden):
    from oxmpl_amd.base import ProblemDefinition, SE3RigidBodyValidityChecker, SE3State, SE3StateSpace
    from oxmpl_amd.geometric import RRTConnect

    class Goal:
        def __init__(self, target, radius):
            self.target, self.radius = target, radius

    sc = scene(se3_golden, "field")
    fsc = scenarios.se3_field()                                  # the package's own scene is the golden file's
    assert np.array_equal(bits(fsc["spheres"][0]), bits([c for c, _ in sc["obstacles"]]))
    assert np.array_equal(bits(fsc["spheres"][1]), bits([r for _, r in sc["obstacles"]]))
    assert np.array_equal(bits(fsc["start"]), bits(sc["start"])) and np.array_equal(bits(fsc["goal_centre"]), bits(sc["target"]))
    space = SE3StateSpace(sc["bounds_xyz"])
    start, target = SE3State.from_values(sc["start"]), SE3State.from_values(sc["target"])
    assert bits(space.distance(start, target)) == bits(se3.distance(sc["start"], sc["target"]))
    pd = ProblemDefinition.from_se3(space, start, Goal(target, sc["goal_r"]))
    planner = RRTConnect(sc["max_distance"], sc["goal_bias"], pd, seed=42, problem_id=0)
    planner.setup(SE3RigidBodyValidityChecker(sc["body"], sc["obstacles"]))
    assert planner.is_state_valid(start)
    path = planner.solve(60.0)
    res = se3.run_scene(sc, 42, 0)
    assert all(isinstance(s, SE3State) for s in path.states)
    assert np.array_equal(bits([s.values for s in path.states]), bits(_rows(res["path"])))
    assert planner.num_nodes == sum(res["n"])
    # the batch builder of the package's scenes
    b = scenarios.make_se3_batch(scenarios.se3_slot(), 4)
    assert (b.solve(BUDGET) == capi.OK).all()
    rows = se3.count_rows(se3_golden["slot"])
    assert [int(v) for v in b.counts()["checksum"]] == [int(r[3], 16) for r in rows[:4]]
    b.close()


def test_body_and_obstacle_argument_checks(se3_golden):
    sc = scene(se3_golden, "field")
    g = make_gpu(sc, 1, 0, 0)
    for centres, radii in (([[0.0] * 3] * 17, [0.1] * 17), ([[0.0] * 3], [-0.1]), ([[0.0] * 3], [math.inf]), ([[0.0] * 3], [math.nan]),
                           ([[math.nan, 0.0, 0.0]], [0.1]), ([[0.0, math.inf, 0.0]], [0.1])):
        with pytest.raises(capi.OxhipError) as ei:
            g.set_body(centres, radii)
        assert ei.value.status == capi.ERR_BAD_ARG, (centres, radii)
    c3, r1 = np.zeros(3), np.zeros(1)
    assert capi.lib().oxhip_rrt_batch_set_body(g._h, capi._p(c3), capi._p(r1), 0) == capi.ERR_BAD_ARG   # an empty body
    with pytest.raises(capi.OxhipError) as ei:
        g.set_boxes([[0.0] * 7], [[1.0] * 7])
    assert ei.value.status == capi.ERR_BAD_ARG
    with pytest.raises(capi.OxhipError) as ei:
        g.set_segments([[0.0, 0.0, 1.0, 1.0]], 0.1)
    assert ei.value.status == capi.ERR_BAD_ARG
    g.solve(BUDGET)                                              # the refused calls left the batch as it was
    assert_same(g, 0, se3.run_scene(sc, 0, 0))
    g.close()
    r3 = capi.RRTBatch(3, [(0.0, 1.0)] * 3, 0.5, 0.05, 1, 100)   # a body belongs to SE(3) batches only
    with pytest.raises(capi.OxhipError) as ei:
        r3.set_body([[0.0] * 3], [0.1])
    assert ei.value.status == capi.ERR_BAD_ARG
    r3.close()
    g = make_gpu(dict(sc, body=[([0.0, 0.0, 0.0], 0.0)]), 1, 5, 2)   # the default body is the point: not setting it changes nothing
    h = capi.RRTBatch(7, config_bounds(sc), sc["max_distance"], sc["goal_bias"], 1, sc["max_nodes"], sc["fraction"], True, 5, 2, 0,
                      capi.KERNEL_AUTO, capi.PLANNER_RRT_CONNECT, 0.0, capi.SPACE_SE3)
    h.set_spheres([c for c, _ in sc["obstacles"]], [r for _, r in sc["obstacles"]])
    h.setup(sc["start"], sc["target"], sc["goal_r"])
    g.solve(BUDGET)
    h.solve(BUDGET)
    assert int(g.counts()["checksum"][0]) == int(h.counts()["checksum"][0])
    assert np.array_equal(bits(g.path(0)), bits(h.path(0)))
    g.close()
    h.close()


def test_stamped_instantiation_computes_the_same(se3_golden):
    for name in ("field", "slot"):
        sc = scene(se3_golden, name)
        rec = se3_golden[name]["runs"][0]
        g = make_gpu(sc, 2, rec["seed"], rec["pid"])
        g.enable_stamps()
        g.solve(BUDGET)
        assert_same(g, 0, from_record(rec))
        w = g.stamps()
        assert int(w[5]) == rec["iterations"] and int(w[5]) <= int(w[6]) <= 2 * int(w[5])      # iterations, extends
        assert all(int(w[k]) > 0 for k in range(5)) and int(w[0]) + int(w[1]) + int(w[2]) + int(w[3]) <= int(w[4])
        g.close()


@pytest.mark.parametrize("flags", [capi.DEBUG_SE3_BRANCHY_SWEEP, capi.DEBUG_SO3_SERIAL_SAMPLER,
                                   capi.DEBUG_SE3_BRANCHY_SWEEP | capi.DEBUG_SO3_SERIAL_SAMPLER])
def test_debug_switches_leave_every_result_as_it_is(se3_golden, flags):
    """the first kernel's pair-by-pair sweep of the motion check and the serial quaternion sampler: same runs, bit for bit"""
    for name in GOLDEN_SCENES:
        sc = scene(se3_golden, name)
        for rec in se3_golden[name]["runs"]:
            g = make_gpu(sc, 1, rec["seed"], rec["pid"], debug_flags=flags)
            g.solve(sc["max_iterations"])
            assert_same(g, 0, from_record(rec))
            g.close()
    sc = scene(se3_golden, "slot")                               # ... and the motions of the stand-alone hook
    chk = se3.make_body(sc)
    rng = mg.ChaCha12Rng(5, 5)
    g = make_gpu(sc, 1, 0, 0, debug_flags=flags)
    frm = [se3.sample_uniform(rng, sc["bounds_xyz"], [0.0, 0.0, 0.0, 1.0], se3.PI) for _ in range(200)]
    for s in frm:
        s[0], s[2] = s[0] * 0.2, s[2] * 0.05
    to = [se3.interpolate(a, se3.sample_uniform(rng, sc["bounds_xyz"], [0.0, 0.0, 0.0, 1.0], se3.PI), 0.1) for a in frm]
    want = [se3.check_motion(chk, sc["bounds_xyz"], sc["fraction"], a, b) for a, b in zip(frm, to)]
    assert g.check_motion(np.array(frm), np.array(to)).tolist() == want and set(want) == {True, False}
    g.close()
