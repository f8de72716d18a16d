#!/usr/bin/env python3
"""Golden vectors for RRTConnect over SE(3) (OXHIP_SPACE_SE3, rrt_connect_se3.hip): an independent pure-Python restatement, the
CPU checker of the SE(3) tests, run to (re)generate tests/golden/se3_golden.json.

The reference has no SE(3) space (docs/BACKLOG.md:12-14 lists it as a next space); the build defines it from the reference's
component spaces, combined the way SE(2) was (make_golden_se2.py) with OMPL's SE(3) weights:
  state          (x, y, z, qx, qy, qz, qw); the quaternion is a unit quaternion, normalising it is the caller's job
  distance       1.0 * RealVectorStateSpace distance of (x, y, z) + 1.0 * SO3StateSpace distance of q      (make_golden.distance,
                 make_golden_so3.distance), one binary64 add
  interpolate    (x, y, z): from + (to - from) * t; q: make_golden_so3.interpolate; the same t
  sample_uniform x, y, z by random_range, then SO(3)'s rejection sampler (make_golden_so3.sample_uniform)
  extent         extent of the (x, y, z) bounds + 0.5 * PI; lvsl = extent * fraction; check_motion steps of lvsl * 0.1
  validity       a rigid body of spheres (c_b, r_b) among world spheres (o_j, r_j): with p = rot(q, c_b) + (x, y, z),
                 valid iff sqrt(|p - o_j|^2) > r_b + r_j for every pair (strict)
  rot(q, v)      u = (qx, qy, qz), w = qw:  t = 2 * (u x v);  rot = (v + w * t) + (u x t), every cross product component a*b - c*d
  planner        rrt_connect.rs:86-309 as make_golden_se2.se2_connect_solve restates it, its checksum folds over seven coordinates
Python floats are IEEE binary64, every operation rounded once, never fused.  PARITY UNPINNED against oxmpl (the space does not
exist there).

    python tests/golden/make_golden_se3.py      (writes tests/golden/se3_golden.json; minutes, 16 worker processes at most)
"""
import json
import math
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (ChaCha12Rng, random_bool, random_range, num_steps, distance, interpolate, hexf)
import make_golden_so3 as s3  # noqa: E402  (distance, interpolate, sample_uniform, space_bounds)

PI = 3.14159265358979323846
M64 = 0xFFFFFFFFFFFFFFFF


# ----------------------------------------------------------------------------------------------------------- SE(3) space
def rot(q, v):
    """rotate v by the unit quaternion q = (x, y, z, w)"""
    x, y, z, w = q
    tx = 2.0 * (y * v[2] - z * v[1])
    ty = 2.0 * (z * v[0] - x * v[2])
    tz = 2.0 * (x * v[1] - y * v[0])
    return [v[0] + w * tx + (y * tz - z * ty), v[1] + w * ty + (z * tx - x * tz), v[2] + w * tz + (x * ty - y * tx)]


def distance(a, b):
    return mg.distance(a[:3], b[:3]) + s3.distance(a[3:], b[3:])


def interpolate(frm, to, t):
    return mg.interpolate(frm[:3], to[:3], t) + s3.interpolate(frm[3:], to[3:], t)


def extent(bounds_xyz):
    return mg.maximum_extent(bounds_xyz) + 0.5 * PI


def lvsl(bounds_xyz, fraction):
    f = fraction if 0.0 < fraction <= 1.0 else (0.0 if fraction <= 0.0 else 1.0)
    return extent(bounds_xyz) * f


def sample_uniform(rng, bounds_xyz, centre, max_angle):
    xyz = [mg.random_range(rng, lo, hi) for lo, hi in bounds_xyz]
    return xyz + s3.sample_uniform(rng, centre, max_angle)


def body_centre(s, c):
    r = rot(s[3:], c)
    return [r[0] + s[0], r[1] + s[1], r[2] + s[2]]


class RigidBody:
    """body: [(centre[3], radius)] in the body frame; obstacles: [(centre[3], radius)] in the world"""

    def __init__(self, body=None, obstacles=()):
        self.body = [([float(v) for v in c], float(r)) for c, r in (body if body is not None else [([0.0, 0.0, 0.0], 0.0)])]
        self.obstacles = [([float(v) for v in c], float(r)) for c, r in obstacles]
        oc = np.array([c for c, _ in self.obstacles], dtype=np.float64).reshape(-1, 3)
        self._ox, self._oy, self._oz = oc[:, 0][None, :], oc[:, 1][None, :], oc[:, 2][None, :]
        rb = np.array([r for _, r in self.body], dtype=np.float64)[:, None]
        ro = np.array([r for _, r in self.obstacles], dtype=np.float64)[None, :]
        self._sum = rb + ro   # r_b + r_j, one binary64 add each

    def is_valid(self, s):
        """the conjunction over all (body sphere, obstacle) pairs, evaluated pair-parallel (numpy's element-wise binary64
        operations round once each: the same values as is_valid_scalar)"""
        if not self.obstacles:
            return True
        p = [body_centre(s, c) for c, _ in self.body]
        dx = np.array([v[0] for v in p])[:, None] - self._ox
        dy = np.array([v[1] for v in p])[:, None] - self._oy
        dz = np.array([v[2] for v in p])[:, None] - self._oz
        acc = dx * dx
        acc = acc + dy * dy
        acc = acc + dz * dz
        return bool(np.all(np.sqrt(acc) > self._sum))

    def is_valid_scalar(self, s):
        for c, rb in self.body:
            p = body_centre(s, c)
            for o, ro in self.obstacles:
                if not (mg.distance(p, o) > rb + ro):
                    return False
        return True


def check_motion(body, bounds_xyz, fraction, frm, to):
    """rrt_connect.rs:166-189"""
    n = mg.num_steps(distance(frm, to), lvsl(bounds_xyz, fraction))
    if n <= 1:
        return body.is_valid(to)
    for i in range(1, n + 1):
        if not body.is_valid(interpolate(frm, to, float(i) / float(n))):
            return False
    return True


def is_path_valid(path, body, bounds_xyz, fraction):
    """is_path_valid of rrt_connect_so3ss_tests.rs:107-142 with the SE(3) distance / interpolate"""
    seg = lvsl(bounds_xyz, fraction)
    for i in range(len(path) - 1):
        a, b = path[i], path[i + 1]
        if not body.is_valid(a):
            return False
        if i + 1 == len(path) - 1 and not body.is_valid(b):
            return False
        n = int(math.ceil(distance(a, b) / seg))
        if n > 1:
            for j in range(1, n + 1):
                if not body.is_valid(interpolate(a, b, float(j) / float(n))):
                    return False
    return True


def connect_solve(bounds_xyz, rot_bounds, max_distance, goal_bias, fraction, body, start, target, goal_r, seed, pid,
                  max_iterations, max_nodes):
    """RRTConnect::solve (rrt_connect.rs:227-309); the goal tree is rooted at sample_goal() = the target"""
    centre, max_angle = s3.space_bounds(rot_bounds)
    rng = mg.ChaCha12Rng(seed, pid)
    trees = [[[float(v) for v in start]], [[float(v) for v in target]]]
    parents = [[-1], [-1]]
    chk = mg.FNV_BASIS
    iterations = 0
    end = [-1, -1]
    target = trees[1][0]

    def extend(w, q):
        tree = trees[w]
        nearest, min_dist = 0, distance(tree[0], q)
        for i in range(1, len(tree)):
            d = distance(tree[i], q)
            if d < min_dist:
                nearest, min_dist = i, d
        q_near = tree[nearest]
        if min_dist > max_distance:
            q_new, res = interpolate(q_near, q, max_distance / min_dist), 1
        else:
            q_new, res = list(q), 2
        if not check_motion(body, bounds_xyz, fraction, q_near, q_new):
            return 0, nearest, q_new
        tree.append(q_new)
        parents[w].append(nearest)
        return res, nearest, q_new

    for _ in range(max_iterations):
        if len(trees[0]) >= max_nodes or len(trees[1]) >= max_nodes:
            break
        grow_start = len(trees[0]) <= len(trees[1])
        if mg.random_bool(rng, goal_bias):
            q_rand = list(target)
        else:
            q_rand = sample_uniform(rng, bounds_xyz, centre, max_angle)
        wa = 0 if grow_start else 1
        wb = 1 - wa
        ra, near_a, qa = extend(wa, q_rand)
        for v in (int(grow_start), near_a, *[mg.f64_bits(x) for x in qa], ra):
            chk = ((chk ^ v) * mg.FNV_P) & M64
        iterations += 1
        done = False
        if ra:
            idx_a = len(trees[wa]) - 1
            if grow_start and distance(qa, target) <= goal_r:
                end = [idx_a, -1]
                done = True
            else:
                rb, near_b, qb = extend(wb, qa)
                for v in (near_b, *[mg.f64_bits(x) for x in qb], rb):
                    chk = ((chk ^ v) * mg.FNV_P) & M64
                if rb == 2:
                    end[wa], end[wb] = idx_a, len(trees[wb]) - 1
                    done = True
        if done:
            break
    path, nodes = [], []   # the merged path and, for each of its states, (tree, node index)
    if end[0] >= 0:
        i = end[0]
        while i >= 0:
            nodes.append([0, i])
            i = parents[0][i]
        nodes.reverse()
        if end[1] >= 0:
            i = parents[1][end[1]]
            while i >= 0:
                nodes.append([1, i])
                i = parents[1][i]
        path = [trees[w][i] for w, i in nodes]
    return dict(n=[len(trees[0]), len(trees[1])], iterations=iterations, checksum=chk, end=end, path=path, path_nodes=nodes,
                states=trees, parents=parents, rng_draws=rng.draws)


# ------------------------------------------------------------------------------------------------------------- scenes
H = math.sqrt(0.5)               # sin(PI / 4) = cos(PI / 4): a quarter turn about y is (0, +-H, 0, H)
ROD = [([-1.0 + 0.5 * i, 0.0, 0.0], 0.25) for i in range(5)]
FIELD_SEED = 0x5EED0018


def field_spheres(seed, n, lo, hi, rmin, rmax, keep_clear, margin):
    """n spheres, centres U[lo,hi)^3, radii U[rmin,rmax) via SplitMix64 + the [1,2)-1 transform; a sphere is redrawn when it
    comes within radius + margin of a keep_clear point"""
    st = seed

    def u(a, b):
        nonlocal st
        st, z = mg.splitmix64(st)
        bits = (z >> 12) | 0x3FF0000000000000
        v = struct.unpack("<d", struct.pack("<Q", bits))[0] - 1.0
        return v * (b - a) + a

    out = []
    while len(out) < n:
        c = [u(lo, hi) for _ in range(3)]
        r = u(rmin, rmax)
        if all(mg.distance(c, p) > r + margin for p in keep_clear):
            out.append((c, r))
    return out


def _base(**kw):
    sc = dict(bounds_xyz=[(-5.0, 5.0)] * 3, rot_bounds=None, max_distance=1.0, goal_bias=0.05, fraction=0.05, goal_r=0.25,
              body=ROD, max_nodes=10000, max_iterations=20000)
    sc.update(kw)
    return sc


def field_scene():
    start = [-4.0, -4.0, -4.0, 0.0, H, 0.0, H]
    target = [4.0, 4.0, 4.0, 0.0, -H, 0.0, H]
    return _base(start=start, target=target,
                 obstacles=field_spheres(FIELD_SEED, 64, -4.5, 4.5, 0.3, 0.9, [start[:3], target[:3]], 1.6))


def slot_scene():
    obstacles = [([0.0, float(iy), float(iz)], 0.62) for iy in range(-5, 6) for iz in range(-5, 6) if iz != 0]
    return _base(start=[-4.0, 0.0, 3.0, 0.0, H, 0.0, H], target=[4.0, 0.0, -3.0, 0.0, -H, 0.0, H], obstacles=obstacles)


def small_scenes():
    fld = field_scene()
    tilt = s3.normalise([0.1, 0.2, -0.3, 0.9])
    b16 = [([-1.2 + 0.16 * i, 0.05 * (i % 3), -0.04 * (i % 4)], 0.1 + 0.01 * i) for i in range(16)]
    return dict(
        bias1=dict(fld, goal_bias=1.0, max_iterations=300),
        point=dict(fld, body=[([0.0, 0.0, 0.0], 0.0)]),
        bounded=dict(fld, rot_bounds=(tilt, 1.2), start=fld["start"][:3] + s3.normalise([0.3, -0.2, -0.1, 0.9]),
                     target=fld["target"][:3] + s3.normalise([-0.2, 0.45, -0.5, 0.7]), max_iterations=200),
        b16=dict(fld, body=b16, max_iterations=400),
        n0=dict(fld, obstacles=[], max_iterations=400),
        tiny=dict(fld, max_distance=0.05, max_iterations=25),   # below the resolution (0.0945): every motion is one state
    )


def make_body(sc):
    return RigidBody(sc["body"], sc["obstacles"])


def run_scene(sc, seed, pid, max_iterations=None, max_nodes=None, body=None):
    return connect_solve(sc["bounds_xyz"], sc["rot_bounds"], sc["max_distance"], sc["goal_bias"], sc["fraction"],
                         body or make_body(sc), sc["start"], sc["target"], sc["goal_r"], seed, pid,
                         max_iterations or sc["max_iterations"], max_nodes or sc["max_nodes"])


def hx(row):
    return [mg.hexf(v) for v in row]


def record(res):
    return dict(n=res["n"], iterations=res["iterations"], checksum="%016x" % res["checksum"], end=res["end"],
                rng_draws=res["rng_draws"], path_nodes=res["path_nodes"],   # (the path's states are tree nodes: written once)
                states=[[hx(r) for r in t] for t in res["states"]], parents=[[int(x) for x in pp] for pp in res["parents"]])


def scene_params(sc, obstacles_of=None):
    """obstacles_of: the name of the scene whose obstacles these are (written once in the file)"""
    return dict(bounds_xyz=[hx(b) for b in sc["bounds_xyz"]],
                rot_bounds=None if sc["rot_bounds"] is None else [hx(sc["rot_bounds"][0]), mg.hexf(sc["rot_bounds"][1])],
                max_distance=mg.hexf(sc["max_distance"]), goal_bias=mg.hexf(sc["goal_bias"]), fraction=mg.hexf(sc["fraction"]),
                goal_r=mg.hexf(sc["goal_r"]), start=hx(sc["start"]), target=hx(sc["target"]),
                body=[[hx(c), mg.hexf(r)] for c, r in sc["body"]],
                obstacles=obstacles_of if obstacles_of else [[hx(c), mg.hexf(r)] for c, r in sc["obstacles"]],
                max_nodes=sc["max_nodes"], max_iterations=sc["max_iterations"])


def scene_from_params(p, golden=None):
    """the inverse of scene_params (the tests rebuild a scene from the golden file; `golden`: the file, for obstacles_of)"""
    if isinstance(p["obstacles"], str):
        p = dict(p, obstacles=golden[p["obstacles"]]["params"]["obstacles"])
    uh = lambda s: struct.unpack("<d", struct.pack("<Q", int(s, 16)))[0]  # noqa: E731
    row = lambda r: [uh(v) for v in r]  # noqa: E731
    return dict(bounds_xyz=[tuple(row(b)) for b in p["bounds_xyz"]],
                rot_bounds=None if p["rot_bounds"] is None else (row(p["rot_bounds"][0]), uh(p["rot_bounds"][1])),
                max_distance=uh(p["max_distance"]), goal_bias=uh(p["goal_bias"]), fraction=uh(p["fraction"]), goal_r=uh(p["goal_r"]),
                start=row(p["start"]), target=row(p["target"]), body=[(row(c), uh(r)) for c, r in p["body"]],
                obstacles=[(row(c), uh(r)) for c, r in p["obstacles"]], max_nodes=p["max_nodes"],
                max_iterations=p["max_iterations"])


def dump_compact(out):
    """the file's text: compact JSON, one line per top-level entry, per recorded run and per eight checksums"""
    enc = lambda v: json.dumps(v, sort_keys=True, separators=(",", ":"))  # noqa: E731
    parts = []
    for key in sorted(out):
        v = out[key]
        if isinstance(v, dict) and "runs" in v:
            items = []
            for k in sorted(v):
                if k == "runs":
                    items.append('"runs":[\n' + ",\n".join(enc(r) for r in v[k]) + "]")
                elif k == "counts":   # column-wise (see count_rows): iterations, tree sizes, then the checksums end to end
                    c = v[k]
                    items.append('"counts":{"iterations":' + enc([r[0] for r in c]) + ',\n"start_nodes":' + enc([r[1] for r in c]) +
                                 ',\n"goal_nodes":' + enc([r[2] for r in c]) + ',\n"checksums":[\n' +
                                 ",\n".join('"' + "".join(r[3] for r in c[i:i + 8]) + '"' for i in range(0, len(c), 8)) + "]}")
                else:
                    items.append(enc(k) + ":" + enc(v[k]))
            parts.append(enc(key) + ":{" + ",\n".join(items) + "}")
        else:
            parts.append(enc(key) + ":" + enc(v))
    return "{" + ",\n".join(parts) + "}\n"


def count_rows(entry):
    """the recorded counts of a scene of the golden file as rows [iterations, start-tree nodes, goal-tree nodes, checksum]"""
    c = entry["counts"]
    chk = "".join(c["checksums"])
    return [[c["iterations"][i], c["start_nodes"][i], c["goal_nodes"][i], chk[16 * i:16 * i + 16]] for i in range(len(c["iterations"]))]


COUNT_SEED = 42
N_FIELD, N_SLOT = 1024, 256
_SCENES = {}


def _count_job(job):
    name, pid = job
    if name not in _SCENES:
        sc = field_scene() if name == "field" else slot_scene()
        _SCENES[name] = (sc, make_body(sc))
    sc, body = _SCENES[name]
    r = run_scene(sc, COUNT_SEED, pid, body=body)
    return name, pid, [r["iterations"], r["n"][0], r["n"][1], "%016x" % r["checksum"], int(r["end"][0] >= 0)]


def kats():
    r = mg.ChaCha12Rng(16, 16)
    out = []
    for _ in range(8):
        a = [mg.random_range(r, -10.0, 10.0) for _ in range(3)] + s3.sample_uniform(r, [0.0, 0.0, 0.0, 1.0], PI)
        b = [mg.random_range(r, -10.0, 10.0) for _ in range(3)] + s3.sample_uniform(r, [0.0, 0.0, 0.0, 1.0], PI)
        t = mg.random_range(r, 0.0, 1.0)
        v = [mg.random_range(r, -2.0, 2.0) for _ in range(3)]
        out.append(dict(a=hx(a), b=hx(b), t=mg.hexf(t), v=hx(v), distance=mg.hexf(distance(a, b)),
                        interpolate=hx(interpolate(a, b, t)), rot=hx(rot(a[3:], v)), body_centre=hx(body_centre(a, v))))
    return out


def main():
    from multiprocessing import Pool
    out = {"_generator": "tests/golden/make_golden_se3.py",
           "_parity": "UNPINNED: SE(3) does not exist in the reference; it is assembled from the reference's R^3 and SO(3) spaces"}
    out["kat"] = dict(random=kats(), extent=mg.hexf(extent([(-5.0, 5.0)] * 3)))
    fld, slt = field_scene(), slot_scene()
    assert make_body(fld).is_valid(fld["start"]) and make_body(fld).is_valid(fld["target"])
    assert make_body(slt).is_valid(slt["start"]) and make_body(slt).is_valid(slt["target"])
    jobs = [("slot", i) for i in range(N_SLOT)] + [("field", i) for i in range(N_FIELD)]
    with Pool(min(16, os.cpu_count() or 1)) as pool:
        res = pool.map(_count_job, jobs, chunksize=1)
    counts = {"field": [None] * N_FIELD, "slot": [None] * N_SLOT}
    for name, pid, row in res:
        counts[name][pid] = row
    for name, sc in (("field", fld), ("slot", slt)):
        rows = counts[name]
        assert all(r[4] == 1 for r in rows), (name, [i for i, r in enumerate(rows) if r[4] != 1])   # every problem is solved
        if name == "field":
            pairs = [(COUNT_SEED, 0), (7, 3)]
        else:   # the two problems with the smallest trees
            order = sorted(range(N_SLOT), key=lambda i: (rows[i][1] + rows[i][2], i))
            pairs = [(COUNT_SEED, order[0]), (COUNT_SEED, order[1])]
        runs = []
        for seed, pid in pairs:
            rec = record(run_scene(sc, seed, pid))
            rec.update(seed=seed, pid=pid)
            runs.append(rec)
        out[name] = dict(params=scene_params(sc), runs=runs, count_seed=COUNT_SEED, counts=[r[:4] for r in rows])
    for name, sc in small_scenes().items():
        runs = []
        for seed, pid in ((7, 3),):   # (the field's second pair: the point body's run is compared with the rod's)
            rec = record(run_scene(sc, seed, pid))
            rec.update(seed=seed, pid=pid)
            runs.append(rec)
        out[name] = dict(params=scene_params(sc, "field" if sc["obstacles"] == fld["obstacles"] else None), runs=runs)
    path = os.path.join(HERE, "se3_golden.json")
    with open(path, "w") as f:
        f.write(dump_compact(out))
    print("wrote", path, os.path.getsize(path), "bytes")
    for name in ("field", "slot"):
        its = sorted(r[0] for r in counts[name])
        print(name, "iterations min / median / max", its[0], its[len(its) // 2], its[-1], "largest tree",
              max(max(r[1], r[2]) for r in counts[name]))
    for k, v in out.items():
        if isinstance(v, dict) and "runs" in v:
            print(k, [(r["seed"], r["pid"], r["n"], r["iterations"], r["end"], len(r["path_nodes"])) for r in v["runs"]])


if __name__ == "__main__":
    main()
