#!/usr/bin/env python3
"""Golden vectors for RRT over SO2StateSpace (OXHIP_SPACE_SO2, rrt_so2.hip): an independent pure-Python restatement, the CPU
checker of the SO(2) tests, run to (re)generate tests/golden/so2_golden.json.

What it restates (Python floats are IEEE binary64, every operation rounded once, never fused; math.fmod is C's fmod: exact):
  state / space   oxmpl/src/base/states/so2_state.rs (new / normalise: (v + PI).rem_euclid(2 PI) - PI),
                  oxmpl/src/base/spaces/so2_state_space.rs: new :57-74 (lo >= hi refused, clamped to [-PI, PI]); distance :97-101;
                  interpolate :107-122 (the shortest way round on the normalised ends, from.value + diff * t on the un-normalised
                  `from`, then normalise); sample_uniform (random_range(lo..hi)); extent PI, lvsl = PI * fraction
  checker / goal  oxmpl/tests/rrt_so2ss_tests.rs: ForbiddenAngleChecker (!(min <= normalise(v) <= max)), generalised to several
                  arcs; the goal (distance(s, target) <= radius; sample_goal = the target: OXHIP_GOAL_SAMPLE_CENTRE)
  planner         oxmpl/src/geometric/planners/rrt.rs:90-128, 170-225 and the per-iteration checksum of ABI 2
The RNG, rand's transforms, num_steps and the checksum's constants are make_golden.py's.  Everything here is add, subtract,
multiply, divide and fmod: apart from the RNG stream (build-defined), a rustc-built oxmpl computes the same bits.

    python tests/golden/make_golden_so2.py      (writes tests/golden/so2_golden.json)
"""
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (ChaCha12Rng, random_bool, random_range, num_steps, f64_bits, hexf, FNV constants)

PI = 3.14159265358979323846
M64 = 0xFFFFFFFFFFFFFFFF


# ------------------------------------------------------------------------------------------------------------- the space
def rem_euclid_2pi(a):
    """f64::rem_euclid(a, 2 PI): r = a % b; if r < 0.0 { r + b } else { r }"""
    b = 2.0 * PI
    r = float("nan") if math.isinf(a) else math.fmod(a, b)
    return r + b if r < 0.0 else r


def normalise(v):
    return rem_euclid_2pi(v + PI) - PI


def distance(a, b):
    diff = a - b
    diff = rem_euclid_2pi(diff + PI) - PI
    return abs(diff)


def interpolate(frm, to, t):
    d = normalise(to) - normalise(frm)
    if d > PI:
        d -= 2.0 * PI
    elif d < -PI:
        d += 2.0 * PI
    return normalise(frm + d * t)


def space_bounds(bounds):
    """SO2StateSpace::new: None = the full circle; lo >= hi is InvalidBound; clamped to [-PI, PI]"""
    lo, hi = (-PI, PI) if bounds is None else bounds
    if lo >= hi:
        raise ValueError("InvalidBound")
    return max(lo, -PI), min(hi, PI)


class Arcs:
    """ForbiddenAngleChecker generalised to several arcs: valid iff the normalised value lies in no closed arc [min, max]"""

    def __init__(self, arcs=()):
        self.arcs = [(float(lo), float(hi)) for lo, hi in arcs]

    def is_valid(self, v):
        nv = normalise(v)
        return not any(lo <= nv <= hi for lo, hi in self.arcs)


def lvsl(fraction):
    f = fraction if 0.0 < fraction <= 1.0 else (0.0 if fraction <= 0.0 else 1.0)
    return PI * f


def motion_states(fraction, frm, to):
    """the states check_motion (rrt.rs:90-116) tests, in order"""
    n = mg.num_steps(distance(frm, to), lvsl(fraction))
    if n <= 1:
        return [to]
    return [interpolate(frm, to, float(i) / float(n)) for i in range(1, n + 1)]


def check_motion(arcs, fraction, frm, to):
    """rrt.rs:90-116"""
    n = mg.num_steps(distance(frm, to), lvsl(fraction))
    if n <= 1:
        return arcs.is_valid(to)
    for i in range(1, n + 1):
        if not arcs.is_valid(interpolate(frm, to, float(i) / float(n))):
            return False
    return True


def is_so2_path_valid(path, arcs, fraction=0.05):
    """is_so2_path_valid of rrt_so2ss_tests.rs: every vertex valid, every edge valid discretised at lvsl"""
    seg = lvsl(fraction)
    for i in range(len(path) - 1):
        a, b = path[i], path[i + 1]
        if not arcs.is_valid(a):
            return False
        if i + 1 == len(path) - 1 and not arcs.is_valid(b):
            return False
        n = int(math.ceil(distance(a, b) / seg))
        if n > 1:
            for j in range(1, n + 1):
                if not arcs.is_valid(interpolate(a, b, float(j) / float(n))):
                    return False
    return True


def nearest_node(states, q):
    """rrt.rs:187-196"""
    nearest, min_dist = 0, distance(states[0], q)
    for i in range(1, len(states)):
        d = distance(states[i], q)
        if d < min_dist:
            nearest, min_dist = i, d
    return nearest, min_dist


def rrt_solve(bounds, max_distance, goal_bias, fraction, arcs, start, target, goal_r, seed, pid, max_iterations, max_nodes,
              stop_at_goal=True, freeze=False, tree=None, parents=None, draws=0, trace=None):
    """RRT::solve over SO(2) for at most max_iterations iterations; tree / parents: a warm start (set_tree after setup);
    draws: words of the stream already consumed (a warm start after an earlier solve); trace: a list that receives
    (q_rand, nearest, min_dist, q_new, ok) per iteration"""
    lo, hi = space_bounds(bounds)
    rng = mg.ChaCha12Rng(seed, pid)
    for _ in range(draws):
        rng.next_u64()
    states = [float(s) for s in tree] if tree is not None else [float(start)]
    par = list(parents) if parents is not None else [-1]
    chk = mg.FNV_BASIS
    iterations = accepted = 0
    goal_node = -1
    for _ in range(max_iterations):
        if (not freeze) and len(states) >= max_nodes:
            break
        if mg.random_bool(rng, goal_bias):
            q = float(target)
        else:
            q = mg.random_range(rng, lo, hi)
        nearest, min_dist = nearest_node(states, q)
        q_near = states[nearest]
        q_new = interpolate(q_near, q, max_distance / min_dist) if min_dist > max_distance else q
        ok = check_motion(arcs, fraction, q_near, q_new)
        if trace is not None:
            trace.append((q, nearest, min_dist, q_new, ok))
        g = ((mg.FNV_BASIS ^ nearest) * mg.FNV_P) & M64
        g = ((g ^ mg.f64_bits(q_new)) * mg.FNV_P) & M64
        g = ((g ^ int(ok)) * mg.FNV_P) & M64
        chk = (chk * mg.FNV_P + g) & M64
        iterations += 1
        hit = False
        if ok:
            accepted += 1
            if not freeze:
                states.append(q_new)
                par.append(nearest)
                if distance(q_new, target) <= goal_r:
                    if goal_node < 0:
                        goal_node = len(states) - 1
                    hit = True
        if hit and stop_at_goal:
            break
    path = []
    if goal_node >= 0:
        i = goal_node
        while i >= 0:
            path.append(states[i])
            i = par[i]
        path.reverse()
    return dict(n=len(states), iterations=iterations, accepted=accepted, checksum=chk, goal_node=goal_node, states=states,
                parents=par, path=path, rng_draws=rng.draws)


# ------------------------------------------------------------------------------------------------------------- scenes
def fixture_scene():
    """test_rrt_finds_path_in_so2ss (rrt_so2ss_tests.rs): the full circle, SO2State::new(-PI / 2) to SO2State::new(PI / 2) with
    radius 0.1, the arc [-0.5, 0.5] forbidden, RRT::new(0.2, 0.05), fraction 0.05: ceil(0.2 / (PI * 0.05 * 0.1)) = 13 states per
    full step"""
    return dict(bounds=None, max_distance=0.2, goal_bias=0.05, fraction=0.05, start=normalise(-PI / 2.0),
                target=normalise(PI / 2.0), goal_r=0.1, arcs=[(-0.5, 0.5)], max_nodes=10000, max_iterations=20000)


def scenes():
    fx = fixture_scene()
    bounded = dict(bounds=(-2.5, 2.8), max_distance=0.3, goal_bias=0.05, fraction=0.05, start=-2.0, target=1.6, goal_r=0.1,
                   arcs=[(-1.2, -1.0), (-0.6, -0.2), (0.9, 1.1)], max_nodes=4000, max_iterations=3000)
    bias1 = dict(fx, goal_bias=1.0, max_iterations=300)
    blocked = dict(fx, arcs=[(-4.0, 4.0)], max_iterations=200)   # every state is forbidden: no motion is ever accepted
    tiny = dict(bounds=(-1.0, 2.0), max_distance=0.01, goal_bias=0.05, fraction=0.02, start=0.1, target=1.5, goal_r=0.05,
                arcs=[(-0.3, -0.2)], max_nodes=1000, max_iterations=400)
    return dict(fixture=fx, bounded=bounded, bias1=bias1, blocked=blocked, tiny=tiny)


def run_scene(sc, seed, pid, max_iterations=None, **kw):
    return rrt_solve(sc["bounds"], sc["max_distance"], sc["goal_bias"], sc["fraction"], Arcs(sc["arcs"]), sc["start"],
                     sc["target"], sc["goal_r"], seed, pid, max_iterations or sc["max_iterations"], sc["max_nodes"], **kw)


def record(res):
    return dict(n=res["n"], iterations=res["iterations"], accepted=res["accepted"], checksum="%016x" % res["checksum"],
                goal_node=res["goal_node"], rng_draws=res["rng_draws"], states=[mg.hexf(v) for v in res["states"]],
                parents=[int(p) for p in res["parents"]], path=[mg.hexf(v) for v in res["path"]])


def scene_params(sc):
    return dict(bounds=None if sc["bounds"] is None else [mg.hexf(v) for v in sc["bounds"]],
                max_distance=mg.hexf(sc["max_distance"]), goal_bias=mg.hexf(sc["goal_bias"]), fraction=mg.hexf(sc["fraction"]),
                start=mg.hexf(sc["start"]), target=mg.hexf(sc["target"]), goal_r=mg.hexf(sc["goal_r"]),
                arcs=[[mg.hexf(lo), mg.hexf(hi)] for lo, hi in sc["arcs"]], max_nodes=sc["max_nodes"],
                max_iterations=sc["max_iterations"])


def main():
    out = {"_generator": "tests/golden/make_golden_so2.py",
           "_parity": "the arithmetic is add, subtract, multiply, divide and fmod: bit-identical to a rustc-built oxmpl; only the "
                      "RNG stream (ChaCha12 keyed by (seed, problem id)) is this build's own"}
    for name, sc in scenes().items():
        runs = []
        for seed, pid in ((0, 0), (7, 3)):
            rec = record(run_scene(sc, seed, pid))
            rec.update(seed=seed, pid=pid)
            runs.append(rec)
        out[name] = dict(params=scene_params(sc), runs=runs)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "so2_golden.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
    print("wrote", path, {k: [(r["n"], r["iterations"], r["accepted"], r["goal_node"], r["rng_draws"]) for r in v["runs"]]
                          for k, v in out.items() if isinstance(v, dict) and "runs" in v})


if __name__ == "__main__":
    main()
