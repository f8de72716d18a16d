#!/usr/bin/env python3
"""Golden vectors for RRT over SO3StateSpace (OXHIP_SPACE_SO3, rrt_so3.hip): an independent pure-Python restatement, the CPU
checker of the SO(3) tests, run to (re)generate tests/golden/so3_golden.json.

What it restates (Python floats are IEEE binary64, every operation rounded once, never fused):
  state / space   oxmpl/src/base/states/so3_state.rs, oxmpl/src/base/spaces/so3_state_space.rs
                  distance :101-110 (abs_dot > 1 - 1e-9 ? 0 : acos(abs_dot)); interpolate :117-159 (LERP + normalise when the
                  sign-flipped dot exceeds 0.9995, else SLERP); sample_uniform :201-231 (four random_range(-1.0..1.0) words per
                  rejection attempt); extent 0.5 * PI, lvsl = extent * fraction :81-84, :234-236
  checker / goal  oxmpl/tests/rrt_so3ss_tests.rs: ForbiddenConeChecker (distance(centre, q) > radius), the goal ball
                  (distance(q, target) <= radius, sample_goal = the target: OXHIP_GOAL_SAMPLE_CENTRE), quaternion_from_axis_angle
  planner         oxmpl/src/geometric/planners/rrt.rs:90-128, 170-225 and the per-iteration checksum of ABI 2
acos is ox_acos (FreeBSD msun's e_acos.c in unfused steps, oxmpl_amd/csrc/ox_acos.hpp) and sin / cos are ox_sincos
(make_golden_disc.py), the portable routines the device evaluates; the RNG and rand's transforms are make_golden.py's.  Against
a rustc-built oxmpl, whose acos / sin are the host libm's, every evaluation is within a few ulp: PARITY UNPINNED.

    python tests/golden/make_golden_so3.py      (writes tests/golden/so3_golden.json)
"""
import json
import math
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (ChaCha12Rng, random_bool, random_range, f64_bits, hexf, FNV constants)
from make_golden_disc import ox_sincos  # noqa: E402

PI = 3.14159265358979323846
M64 = 0xFFFFFFFFFFFFFFFF


# ------------------------------------------------------------------------------------------------------------- ox_acos
def _hi(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0] >> 32


def _lo(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0] & 0xFFFFFFFF


def _from_hi(h):
    return struct.unpack("<d", struct.pack("<Q", h << 32))[0]


PS0, PS1, PS2 = 1.66666666666666657415e-01, -3.25565818622400915405e-01, 2.01212532134862925881e-01
PS3, PS4, PS5 = -4.00555345006794114027e-02, 7.91534994289814532176e-04, 3.47933107596021167570e-05
QS1, QS2, QS3, QS4 = -2.40339491173441421878e+00, 2.02094576023350569471e+00, -6.88283971605453293030e-01, 7.70381505559019352791e-02
ACOS_PI, PIO2_HI, PIO2_LO = 3.14159265358979311600e+00, 1.57079632679489655800e+00, 6.12323399573676603587e-17


def _acos_r(z):
    p = z * (PS0 + z * (PS1 + z * (PS2 + z * (PS3 + z * (PS4 + z * PS5)))))
    q = 1.0 + z * (QS1 + z * (QS2 + z * (QS3 + z * QS4)))
    return p / q


def ox_acos(x):
    x = float(x)
    h = _hi(x)
    ix, neg = h & 0x7FFFFFFF, h >> 31
    if ix >= 0x3FF00000:
        if ix == 0x3FF00000 and _lo(x) == 0:
            return ACOS_PI + 2.0 * PIO2_LO if neg else 0.0
        return float("nan")
    if ix < 0x3FE00000:
        if ix <= 0x3C600000:
            return PIO2_HI + PIO2_LO
        z = x * x
        r = _acos_r(z)
        return PIO2_HI - (x - (PIO2_LO - x * r))
    if neg:
        z = (1.0 + x) * 0.5
        s = math.sqrt(z)
        r = _acos_r(z)
        w = r * s - PIO2_LO
        return ACOS_PI - 2.0 * (s + w)
    z = (1.0 - x) * 0.5
    s = math.sqrt(z)
    df = _from_hi(_hi(s))
    c = (z - df * df) / (s + df)
    r = _acos_r(z)
    w = r * s + c
    return 2.0 * (df + w)


def ox_sin(x):
    return ox_sincos(x)[0]


# ----------------------------------------------------------------------------------------------------------- SO(3) space
def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3]


def distance(a, b):
    abs_dot = abs(dot(a, b))
    return 0.0 if abs_dot > 1.0 - 1e-9 else ox_acos(abs_dot)


def interpolate(frm, to, t):
    d = dot(frm, to)
    sign = -1.0 if d < 0.0 else 1.0
    d = d * sign
    if d > 0.9995:
        o = [frm[k] + t * (to[k] * sign - frm[k]) for k in range(4)]
        norm = math.sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2] + o[3] * o[3])
        return [v / norm for v in o]
    theta = ox_acos(d)
    sin_theta = ox_sin(theta)
    s0 = ox_sin((1.0 - t) * theta) / sin_theta
    s1 = ox_sin(t * theta) / sin_theta * sign
    return [frm[k] * s0 + to[k] * s1 for k in range(4)]


def space_bounds(bounds):
    """SO3StateSpace::new: None -> (identity, PI); a negative max_angle is an error; clamped to PI (NaN -> PI, f64::min)"""
    if bounds is None:
        return [0.0, 0.0, 0.0, 1.0], PI
    centre, max_angle = [float(v) for v in bounds[0]], float(bounds[1])
    if max_angle < 0.0:
        raise ValueError("max_angle must not be negative")
    return centre, (PI if math.isnan(max_angle) else min(max_angle, PI))


def sample_uniform(rng, centre, max_angle):
    if max_angle < 1e-9:
        return list(centre)
    while True:
        v = [mg.random_range(rng, -1.0, 1.0) for _ in range(4)]
        norm_sq = v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]
        if norm_sq > 1e-9 and norm_sq < 1.0:
            norm = math.sqrt(norm_sq)
            q = [x / norm for x in v]
            if distance(centre, q) <= max_angle:
                return q


def quaternion_from_axis_angle(axis, angle):
    """the fixture's helper (rrt_so3ss_tests.rs:17-43) with ox_sincos for sin / cos"""
    norm = math.sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2])
    if norm < 1e-9:
        return [0.0, 0.0, 0.0, 1.0]
    u = [a / norm for a in axis]
    half = angle * 0.5
    s, c = ox_sincos(half) if half >= 0.0 else (lambda sc: (-sc[0], sc[1]))(ox_sincos(-half))
    return [u[0] * s, u[1] * s, u[2] * s, c]


def normalise(q):
    norm = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return [v / norm for v in q]


class Cones:
    """ForbiddenConeChecker generalised to several cones: valid iff distance(centre, q) > radius for every cone"""

    def __init__(self, cones=()):
        self.cones = [([float(v) for v in c], float(r)) for c, r in cones]

    def is_valid(self, q):
        return all(distance(c, q) > r for c, r in self.cones)


def lvsl(fraction):
    f = fraction if 0.0 < fraction <= 1.0 else (0.0 if fraction <= 0.0 else 1.0)
    return 0.5 * PI * f


def check_motion(cones, fraction, frm, to):
    """rrt.rs:90-116"""
    n = mg.num_steps(distance(frm, to), lvsl(fraction))
    if n <= 1:
        return cones.is_valid(to)
    for i in range(1, n + 1):
        if not cones.is_valid(interpolate(frm, to, float(i) / float(n))):
            return False
    return True


def is_so3_path_valid(path, cones, fraction=0.05):
    """is_path_valid of rrt_so3ss_tests.rs:108-143: every vertex valid, every edge valid discretised at lvsl"""
    seg = lvsl(fraction)
    for i in range(len(path) - 1):
        a, b = path[i], path[i + 1]
        if not cones.is_valid(a):
            return False
        if i + 1 == len(path) - 1 and not cones.is_valid(b):
            return False
        d = distance(a, b)
        n = int(math.ceil(d / seg))
        if n > 1:
            for j in range(1, n + 1):
                if not cones.is_valid(interpolate(a, b, float(j) / float(n))):
                    return False
    return True


def rrt_solve(bounds, max_distance, goal_bias, fraction, cones, start, target, goal_r, seed, pid, max_iterations, max_nodes,
              stop_at_goal=True, freeze=False, tree=None, parents=None, draws=0):
    """RRT::solve over SO(3) for at most max_iterations iterations; tree / parents: a warm start (set_tree after setup);
    draws: words of the stream already consumed (a warm start after an earlier solve)"""
    centre, max_angle = space_bounds(bounds)
    rng = mg.ChaCha12Rng(seed, pid)
    for _ in range(draws):
        rng.next_u64()
    states = [list(map(float, s)) for s in tree] if tree is not None else [list(map(float, start))]
    par = list(parents) if parents is not None else [-1]
    chk = mg.FNV_BASIS
    iterations = accepted = 0
    goal_node = -1
    for _ in range(max_iterations):
        if (not freeze) and len(states) >= max_nodes:
            break
        if mg.random_bool(rng, goal_bias):
            q = list(target)
        else:
            q = sample_uniform(rng, centre, max_angle)
        nearest, min_dist = 0, distance(states[0], q)
        for i in range(1, len(states)):
            d = distance(states[i], q)
            if d < min_dist:
                nearest, min_dist = i, d
        q_near = states[nearest]
        q_new = interpolate(q_near, q, max_distance / min_dist) if min_dist > max_distance else list(q)
        ok = check_motion(cones, fraction, q_near, q_new)
        g = ((mg.FNV_BASIS ^ nearest) * mg.FNV_P) & M64
        for v in q_new:
            g = ((g ^ mg.f64_bits(v)) * mg.FNV_P) & M64
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
    """test_rrt_finds_path_in_so3ss (rrt_so3ss_tests.rs:145-214): RRT::new(0.5, 0.0), unbounded space, start / goal a quarter
    turn either way about y, goal radius 10 degrees, one forbidden cone of 44.9 degrees about the identity"""
    return dict(bounds=None, max_distance=0.5, goal_bias=0.0, fraction=0.05,
                start=quaternion_from_axis_angle([0.0, 1.0, 0.0], PI / 2.0),
                target=quaternion_from_axis_angle([0.0, 1.0, 0.0], -PI / 2.0),
                goal_r=10.0 * (PI / 180.0), cones=[([0.0, 0.0, 0.0, 1.0], 44.9 * (PI / 180.0))],
                max_nodes=10000, max_iterations=20000)


def scenes():
    fx = fixture_scene()
    c1 = normalise([0.1, 0.2, -0.3, 0.9])
    bounded = dict(bounds=(c1, 1.2), max_distance=0.3, goal_bias=0.05, fraction=0.05,
                   start=normalise([0.3, -0.2, -0.1, 0.9]), target=normalise([-0.35, 0.45, -0.5, 0.65]), goal_r=0.15,
                   cones=[(normalise([-0.03, 0.13, -0.3, 0.78]), 0.25), (normalise([0.1, 0.3, -0.45, 0.8]), 0.15),
                          (normalise([-0.3, 0.1, -0.1, 0.9]), 0.2)],
                   max_nodes=4000, max_iterations=3000)
    bias1 = dict(fx, goal_bias=1.0, max_iterations=300)
    tiny = dict(bounds=(normalise([0.0, 0.0, 0.5, 0.8]), 2.0), max_distance=0.01, goal_bias=0.05, fraction=0.02,
                start=normalise([0.0, 0.1, 0.5, 0.8]), target=normalise([0.5, 0.0, 0.0, 0.8]), goal_r=0.05,
                cones=[(normalise([0.2, 0.05, 0.3, 0.9]), 0.05)], max_nodes=1000, max_iterations=400)
    return dict(fixture=fx, bounded=bounded, bias1=bias1, tiny=tiny)


def run_scene(sc, seed, pid, max_iterations=None, **kw):
    return rrt_solve(sc["bounds"], sc["max_distance"], sc["goal_bias"], sc["fraction"], Cones(sc["cones"]), sc["start"],
                     sc["target"], sc["goal_r"], seed, pid, max_iterations or sc["max_iterations"], sc["max_nodes"], **kw)


def record(res):
    return dict(n=res["n"], iterations=res["iterations"], accepted=res["accepted"], checksum="%016x" % res["checksum"],
                goal_node=res["goal_node"], rng_draws=res["rng_draws"],
                states=[[mg.hexf(v) for v in row] for row in res["states"]], parents=[int(p) for p in res["parents"]],
                path=[[mg.hexf(v) for v in row] for row in res["path"]])


def scene_params(sc):
    hx = lambda row: [mg.hexf(v) for v in row]  # noqa: E731
    return dict(bounds=None if sc["bounds"] is None else [hx(sc["bounds"][0]), mg.hexf(sc["bounds"][1])],
                max_distance=mg.hexf(sc["max_distance"]), goal_bias=mg.hexf(sc["goal_bias"]), fraction=mg.hexf(sc["fraction"]),
                start=hx(sc["start"]), target=hx(sc["target"]), goal_r=mg.hexf(sc["goal_r"]),
                cones=[[hx(c), mg.hexf(r)] for c, r in sc["cones"]], max_nodes=sc["max_nodes"], max_iterations=sc["max_iterations"])


def main():
    out = {"_generator": "tests/golden/make_golden_so3.py",
           "_parity": "UNPINNED: acos / sin are the build's ox_acos / ox_sincos (within one ulp of any libm), rand's transforms are "
                      "restated; the reference cannot be built here"}
    xs = [0.0, 1e-300, 0.25, 0.5, 0.7071067811865476, 0.9995, 0.999999999, 1.0 - 1e-9, 1.0, -0.5, -0.9, -1.0]
    out["acos"] = [dict(x=mg.hexf(x), acos=mg.hexf(ox_acos(x))) for x in xs]
    for name, sc in scenes().items():
        runs = []
        for seed, pid in ((0, 0), (7, 3)):
            rec = record(run_scene(sc, seed, pid))
            rec.update(seed=seed, pid=pid)
            runs.append(rec)
        out[name] = dict(params=scene_params(sc), runs=runs)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "so3_golden.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
    print("wrote", path, {k: [(r["n"], r["iterations"], r["goal_node"]) for r in v["runs"]] for k, v in out.items()
                          if isinstance(v, dict) and "runs" in v})


if __name__ == "__main__":
    main()
