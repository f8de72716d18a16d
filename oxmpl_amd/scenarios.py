"""Synthetic workloads named by BASELINE.json's configs (inputs only; no planner logic).

config 1: README quick-start, R^2, disc obstacle r=2 at the origin, start (-5,-5), goal (5,5) r=0.5
          (oxmpl README.md:147-171, oxmpl-js/examples/simple_2d_planning.js:8-41)
wall    : the reference's own RRT test scene (oxmpl/tests/rrt_rvss_tests.rs:109-159)
config 2: R^3, [0,10]^3, 64 random spheres, start (.5,.5,.5), goal ball (9.5,9.5,9.5) r=0.5
config 4: SE(2) RRTConnect (BASELINE.json configs[3]): [0,10]^2 x [-PI,PI), 64 random quadrilaterals = 256 segments,
          disc robot of radius 0.15, start (0.5,0.5,0), goal ball (9.5,9.5,1.5) r=0.5
se3 field / slot: SE(3) RRTConnect: [-5,5]^3 x SO(3), a rod of five spheres among 64 random spheres
          (field) or through the one open row of a wall of 110 spheres (slot)
config 5: PRM (BASELINE.json configs[4]): R^6, [0,10]^6, 32 random hyperspheres, 50,000 milestones,
          connection radius 2.0, start (1,..,1), goal ball (9,..,9) r=1.5
"""
import struct

import numpy as np

_M64 = 0xFFFFFFFFFFFFFFFF


def _splitmix64(state):
    state = (state + 0x9E3779B97F4A7C15) & _M64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return state, z ^ (z >> 31)


def sphere_field(seed=0x5EED0001, n=64, dim=3, lo=1.0, hi=9.0, rmin=0.3, rmax=0.8, keep_clear=()):
    """n spheres: centres U[lo,hi)^dim, radii U[rmin,rmax) from SplitMix64(seed) through the
    52-bit [1,2)-1 transform; a sphere closer than radius+0.5 to a keep_clear point is redrawn."""
    st = seed

    def u(a, b):
        nonlocal st
        st, z = _splitmix64(st)
        bits = (z >> 12) | 0x3FF0000000000000
        v = struct.unpack("<d", struct.pack("<Q", bits))[0] - 1.0
        return v * (b - a) + a

    cs, rs = [], []
    while len(rs) < n:
        c = [u(lo, hi) for _ in range(dim)]
        r = u(rmin, rmax)
        ok = True
        for p in keep_clear:
            acc = 0.0
            for x, y in zip(c, p):
                acc = acc + (x - y) * (x - y)
            if not (acc ** 0.5 > r + 0.5):
                ok = False
        if ok:
            cs.append(c)
            rs.append(r)
    return np.array(cs, dtype=np.float64), np.array(rs, dtype=np.float64)


def config1():
    return dict(dim=2, bounds=[(-10.0, 10.0), (-10.0, 10.0)], max_distance=0.5, goal_bias=0.05, lvs_fraction=0.05,
                start=[-5.0, -5.0], goal_centre=[5.0, 5.0], goal_radius=0.5,
                spheres=(np.array([[0.0, 0.0]]), np.array([2.0])), boxes=None)


def wall():
    return dict(dim=2, bounds=[(0.0, 10.0), (0.0, 10.0)], max_distance=0.5, goal_bias=0.0, lvs_fraction=0.05,
                start=[1.0, 5.0], goal_centre=[9.0, 5.0], goal_radius=0.5, spheres=None,
                boxes=(np.array([[4.75, 2.0]]), np.array([[5.25, 8.0]])))


# (scale, offset) frames of the SE(2) scenes' (x, y) plane, headings left as they are (tests/test_gpu_se2.py, tools/fuzz_parity.py).
# Offsets (at 4e6 a binary32 coordinate is off by up to 1/8: the screen separates little) and 1e-12 (the heading term decides);
# 1e18 and (2.4e18, -1.2e19) keep |x|, |y| below 2^64 while node distances cross sqrt(FLT_MAX) = 1.8e19, where binary32 squares
# overflow; 1e36 has finite binary32 coordinates; 1e38 puts the start inside binary32's range and the goal beyond it; 1e40, 1e100
# and offset 1e39 lie wholly beyond it.  Offset 1e39 needs a scale of its own: at unit scale x + 10 == x in binary64.
SE2_FRAMES = [(1.0, 1.0e3), (1.0, 1.0e6), (1.0, 4.0e6), (1.0, -5.0e4), (1.0e-12, 0.0), (1.0e18, 0.0), (2.4e18, -1.2e19),
              (1.0e36, 0.0), (1.0e38, 0.0), (1.0e40, 0.0), (1.0e100, 0.0), (1.0e28, 1.0e39)]


def config2():
    start, goal = [0.5, 0.5, 0.5], [9.5, 9.5, 9.5]
    return dict(dim=3, bounds=[(0.0, 10.0)] * 3, max_distance=0.5, goal_bias=0.05, lvs_fraction=0.05,
                start=start, goal_centre=goal, goal_radius=0.5,
                spheres=sphere_field(keep_clear=[start, goal]), boxes=None)


def polygon_soup(seed=0x5EED0003, n_poly=64, lo=0.8, hi=9.2, wmin=0.15, wmax=0.45, keep_clear=(), margin=0.4):
    """n_poly random quadrilaterals (4 segments each): centre U[lo,hi)^2, half-widths U[wmin,wmax), every vertex
    jittered by up to 30 %; polygons too close to a keep_clear point are redrawn.  SplitMix64, no trigonometry."""
    st = seed

    def u(a, b):
        nonlocal st
        st, z = _splitmix64(st)
        bits = (z >> 12) | 0x3FF0000000000000
        v = struct.unpack("<d", struct.pack("<Q", bits))[0] - 1.0
        return v * (b - a) + a

    segs = []
    while len(segs) < 4 * n_poly:
        cx, cy = u(lo, hi), u(lo, hi)
        w, h = u(wmin, wmax), u(wmin, wmax)
        verts = [(cx + sx * w * u(0.7, 1.3), cy + sy * h * u(0.7, 1.3)) for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
        size = 1.3 * max(w, h) * (2.0 ** 0.5)
        if any(((cx - p[0]) ** 2 + (cy - p[1]) ** 2) ** 0.5 <= size + margin for p in keep_clear):
            continue
        for k in range(4):
            a, b = verts[k], verts[(k + 1) % 4]
            segs.append((a[0], a[1], b[0], b[1]))
    return np.array(segs, dtype=np.float64)


def config4():
    start, goal = [0.5, 0.5, 0.0], [9.5, 9.5, 1.5]
    pi = 3.141592653589793
    return dict(dim=3, bounds=[(0.0, 10.0), (0.0, 10.0), (-pi, pi)], max_distance=0.5, goal_bias=0.05, lvs_fraction=0.05,
                start=start, goal_centre=goal, goal_radius=0.5, clearance=0.15,
                segments=polygon_soup(keep_clear=[start, goal]), spheres=None, boxes=None)


def make_se2_batch(sc, n_problems, max_nodes=10000, seed=42, first_problem_id=0, device=0):
    """RRTConnect over SE(2) among sc["segments"] (oxmpl_amd.capi.SPACE_SE2), set up and ready to solve."""
    from .capi import RRTBatch, KERNEL_AUTO, PLANNER_RRT_CONNECT, SPACE_SE2
    b = RRTBatch(3, sc["bounds"], sc["max_distance"], sc["goal_bias"], n_problems, max_nodes, sc["lvs_fraction"], True,
                 seed, first_problem_id, device, KERNEL_AUTO, PLANNER_RRT_CONNECT, 0.0, SPACE_SE2)
    b.set_segments(sc["segments"], sc["clearance"])
    b.setup(sc["start"], sc["goal_centre"], sc["goal_radius"])
    return b


def se3_rod():
    """a rod of five spheres of radius 0.25 at body x = -1, -0.5, 0, 0.5, 1: (centres [5][3], radii [5])"""
    return np.array([[-1.0 + 0.5 * i, 0.0, 0.0] for i in range(5)]), np.full(5, 0.25)


def _se3_scene(start_xyz, goal_xyz, spheres):
    h = 0.5 ** 0.5   # a quarter turn about y either way: (0, +-sin(PI/4), 0, cos(PI/4)), by a square root alone
    return dict(dim=7, bounds=[(-5.0, 5.0)] * 3, rotation_bounds=None, max_distance=1.0, goal_bias=0.05, lvs_fraction=0.05,
                start=list(start_xyz) + [0.0, h, 0.0, h], goal_centre=list(goal_xyz) + [0.0, -h, 0.0, h], goal_radius=0.25,
                body=se3_rod(), spheres=spheres, boxes=None)


def se3_field(seed=0x5EED0018, n=64):
    """n random spheres, radius U[0.3, 0.9), centres U[-4.5, 4.5)^3, none within radius + 1.6 of the start (-4, -4, -4) or
    the target (4, 4, 4).  SplitMix64 + the 52-bit transform, the recipe of sphere_field with its own margin."""
    start, goal = [-4.0, -4.0, -4.0], [4.0, 4.0, 4.0]
    st = seed

    def u(a, b):
        nonlocal st
        st, z = _splitmix64(st)
        bits = (z >> 12) | 0x3FF0000000000000
        v = struct.unpack("<d", struct.pack("<Q", bits))[0] - 1.0
        return v * (b - a) + a

    cs, rs = [], []
    while len(rs) < n:
        c = [u(-4.5, 4.5) for _ in range(3)]
        r = u(0.3, 0.9)
        ok = True
        for p in (start, goal):
            acc = 0.0
            for x, y in zip(c, p):
                acc = acc + (x - y) * (x - y)
            if not (acc ** 0.5 > r + 1.6):
                ok = False
        if ok:
            cs.append(c)
            rs.append(r)
    return _se3_scene(start, goal, (np.array(cs, dtype=np.float64).reshape(-1, 3), np.array(rs, dtype=np.float64)))


def se3_slot():
    """a wall of spheres of radius 0.62 at (0, iy, iz), iy, iz in -5 .. 5, the row iz = 0 left out (110 spheres): the rod
    passes only while it lies near the plane z = 0, so the orientation decides validity"""
    cs = [[0.0, float(iy), float(iz)] for iy in range(-5, 6) for iz in range(-5, 6) if iz != 0]
    return _se3_scene([-4.0, 0.0, 3.0], [4.0, 0.0, -3.0], (np.array(cs, dtype=np.float64), np.full(len(cs), 0.62)))


def se3_config_bounds(sc):
    """the eleven values oxmpl_amd.capi.RRTBatch takes for SPACE_SE3"""
    rb = sc.get("rotation_bounds")
    rot = [0.0, 0.0, 0.0, 1.0, 3.141592653589793] if rb is None else list(rb[0]) + [rb[1]]
    return [v for pair in sc["bounds"] for v in pair] + rot


def make_se3_batch(sc, n_problems, max_nodes=10000, seed=42, first_problem_id=0, device=0, debug_flags=0):
    """RRTConnect over SE(3) for a scene dict (se3_field / se3_slot; oxmpl_amd.capi.SPACE_SE3), set up and ready to solve."""
    from .capi import RRTBatch, KERNEL_AUTO, PLANNER_RRT_CONNECT, SPACE_SE3
    b = RRTBatch(7, se3_config_bounds(sc), sc["max_distance"], sc["goal_bias"], n_problems, max_nodes, sc["lvs_fraction"], True,
                 seed, first_problem_id, device, KERNEL_AUTO, PLANNER_RRT_CONNECT, 0.0, SPACE_SE3, debug_flags=debug_flags)
    if sc.get("body") is not None:
        b.set_body(*sc["body"])
    if sc["spheres"] is not None and len(sc["spheres"][1]):
        b.set_spheres(*sc["spheres"])
    b.setup(sc["start"], sc["goal_centre"], sc["goal_radius"])
    return b


def so2_band():
    """The reference's SO(2) fixture (oxmpl/tests/rrt_so2ss_tests.rs): the full circle, start -PI/2, target PI/2 with radius
    0.1, one forbidden arc [-0.5, 0.5] between them, RRT(0.2, 0.05), fraction 0.05: every path goes round through +-PI."""
    pi = 3.141592653589793
    return dict(dim=1, bounds=(-pi, pi), max_distance=0.2, goal_bias=0.05, lvs_fraction=0.05,
                start=[-pi / 2.0], goal_centre=[pi / 2.0], goal_radius=0.1, arcs=[(-0.5, 0.5)])


def make_so2_batch(sc, n_problems, max_nodes=10000, stop_at_goal=True, seed=42, first_problem_id=0, device=0, kernel=0):
    """RRT over SO(2) among sc["arcs"] (oxmpl_amd.capi.SPACE_SO2), set up and ready to solve."""
    from .capi import RRTBatch, PLANNER_RRT, SPACE_SO2
    b = RRTBatch(1, sc["bounds"], sc["max_distance"], sc["goal_bias"], n_problems, max_nodes, sc["lvs_fraction"], stop_at_goal,
                 seed, first_problem_id, device, kernel, PLANNER_RRT, 0.0, SPACE_SO2)
    b.set_boxes([[lo] for lo, _ in sc["arcs"]], [[hi] for _, hi in sc["arcs"]])
    b.setup(sc["start"], sc["goal_centre"], sc["goal_radius"])
    return b


def config5():
    start, goal = [1.0] * 6, [9.0] * 6
    return dict(dim=6, bounds=[(0.0, 10.0)] * 6, connection_radius=2.0, lvs_fraction=0.05, max_milestones=50000,
                start=start, goal_centre=goal, goal_radius=1.5,
                spheres=sphere_field(seed=0x5EED0005, n=32, dim=6, lo=1.0, hi=9.0, rmin=2.0, rmax=3.5,
                                     keep_clear=[start, goal]), boxes=None)


def make_prm(sc, max_milestones=None, seed=42, stream=0, device=0, timeout=0.0, connection_radius=None, knn_k=0):
    """Build a PRMRoadmap for a scenario dict and run Planner::setup."""
    from .capi import PRMRoadmap
    g = PRMRoadmap(sc["dim"], sc["bounds"], connection_radius or sc["connection_radius"],
                   max_milestones or sc["max_milestones"], timeout, sc["lvs_fraction"], 0, seed, stream, device, knn_k)
    if sc["spheres"] is not None:
        g.set_spheres(*sc["spheres"])
    if sc["boxes"] is not None:
        g.set_boxes(*sc["boxes"])
    g.setup(sc["start"], sc["goal_centre"], sc["goal_radius"])
    return g


def make_batch(sc, n_problems, max_nodes=10000, stop_at_goal=True, seed=42, first_problem_id=0, device=0, kernel=0,
               planner=0, search_radius=0.0, **extra):
    """Build an RRTBatch for a scenario dict and run Planner::setup on every problem."""
    from .capi import RRTBatch
    b = RRTBatch(sc["dim"], sc["bounds"], sc["max_distance"], sc["goal_bias"], n_problems, max_nodes,
                 sc["lvs_fraction"], stop_at_goal, seed, first_problem_id, device, kernel, planner, search_radius, **extra)
    if sc["spheres"] is not None:
        b.set_spheres(*sc["spheres"])
    if sc["boxes"] is not None:
        b.set_boxes(*sc["boxes"])
    b.setup(sc["start"], sc["goal_centre"], sc["goal_radius"])
    return b
