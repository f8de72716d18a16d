"""Constructions for the SE(3) RRTConnect kernel (rrt_connect_se3.hip) at the limits the recorded scenes do
not reach: trees beyond the 256-node LDS mirror (A), motions with exactly one offending (state, body sphere, obstacle) triple, of
up to 129 states (B), pairs at contact and obstacle radii that are not ordinary (C), and frames scaled by 2^-30 / 2^30 (D).

Constructions only, by the checker (tests/golden/make_golden_se3.py) alone: nothing here loads the GPU library.  What
tests/test_gpu_se3_limits.py relies on -- tree sizes, step counts, the one offending triple, both verdicts of a sweep -- is held
on the CPU by tests/test_se3_limits_model.py.  Checker results are computed once (functools caches) and shared: never modify one."""
import functools
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden as mg  # noqa: E402
import make_golden_se3 as se3  # noqa: E402
import make_golden_so3 as so3  # noqa: E402

MIRROR = 256                     # kSe3N: nodes of each tree mirrored in LDS
LDS_OBS = 128                    # kSe3LdsObs: more obstacles take the instantiation that reads them from HBM
POINT = [([0.0, 0.0, 0.0], 0.0)]
B16 = [([-1.2 + 0.16 * i, 0.05 * (i % 3), -0.04 * (i % 4)], 0.1 + 0.01 * i) for i in range(16)]   # the golden b16 layout
BUDGET = 20000


def resolution(sc):
    """the spacing of check_motion's states"""
    return se3.lvsl(sc["bounds_xyz"], sc["fraction"]) * 0.1


def steps(sc, frm, to):
    return mg.num_steps(se3.distance(frm, to), se3.lvsl(sc["bounds_xyz"], sc["fraction"]))


def motion_states(sc, frm, to):
    """the states check_motion tests, in its order"""
    n = steps(sc, frm, to)
    if n <= 1:
        return [list(to)]
    return [se3.interpolate(frm, to, float(i) / float(n)) for i in range(1, n + 1)]


def offending_triples(sc, frm, to):
    """every (state, body sphere, obstacle) of the motion with not (distance > r_b + r_j), states counted from 1; RigidBody.is_valid's
    arithmetic (element-wise binary64, every operation rounded once), all triples enumerated"""
    oc = np.array([c for c, _ in sc["obstacles"]], dtype=np.float64).reshape(-1, 3)
    ro = np.array([r for _, r in sc["obstacles"]], dtype=np.float64)
    rb = np.array([r for _, r in sc["body"]], dtype=np.float64)
    total = rb[:, None] + ro[None, :]
    out = []
    for i, s in enumerate(motion_states(sc, frm, to)):
        p = np.array([se3.body_centre(s, c) for c, _ in sc["body"]], dtype=np.float64)
        dx, dy, dz = p[:, 0:1] - oc[None, :, 0], p[:, 1:2] - oc[None, :, 1], p[:, 2:3] - oc[None, :, 2]
        acc = dx * dx
        acc = acc + dy * dy
        acc = acc + dz * dz
        out.extend((i + 1, int(b), int(j)) for b, j in np.argwhere(~(np.sqrt(acc) > total)))
    return out


def problem_scene(sc, p):
    """problem p of a batch whose problems have their own start and target"""
    return dict(sc, start=sc["start"][p], target=sc["target"][p])


# ------------------------------------------------------------------------------------- A / D: a wall that cannot be crossed
WALL_SEED = 7
WALL_PIDS = (0, 1, 2, 3)
CUT = 97                         # iterations per launch of the resumed run
# problem 0, seed 7: iteration counts after which both trees are below the mirror (a multiple of CUT) / the trees straddle its end,
# min(n) <= 256 <= max(n) with unequal sizes: lds [257, 256], hbm [256, 255]
WALL_BELOW = {"lds": 970, "hbm": 970}
WALL_STRADDLE = {"lds": 1055, "hbm": 1021}
FRAMES = {"down": 2.0 ** -30, "up": 2.0 ** 30}
FRAME_PIDS = (0, 1)


def wall_scene(variant, scale=1.0, max_nodes=300):
    """spheres of radius 0.8 at (0, y, z), y and z integers: `lds` 9 x 9 of them in bounds +-3, a point body; `hbm` 13 x 13 in
    bounds +-5, the first three spheres of the rod.  `scale` (a power of two: exact) multiplies every length."""
    half, bound, body = (4, 3.0, POINT) if variant == "lds" else (6, 5.0, se3.ROD[:3])
    k = float(scale)
    rng = range(-half, half + 1)
    return dict(bounds_xyz=[(-bound * k, bound * k)] * 3, rot_bounds=None, max_distance=0.5 * k, goal_bias=0.05, fraction=0.02,
                goal_r=0.25 * k, body=[([v * k for v in c], r * k) for c, r in body],
                obstacles=[([0.0, y * k, z * k], 0.8 * k) for y in rng for z in rng],
                start=[-2.0 * k, 0.0, 0.0, 0.0, se3.H, 0.0, se3.H], target=[2.0 * k, 0.0, 0.0, 0.0, -se3.H, 0.0, se3.H],
                max_nodes=max_nodes, max_iterations=BUDGET)


@functools.lru_cache(maxsize=None)
def wall_run(variant, pid, max_iterations=None):
    return se3.run_scene(wall_scene(variant), WALL_SEED, pid, max_iterations=max_iterations)


def frame_scene(frame):
    return wall_scene("lds", FRAMES[frame], max_nodes=120)


@functools.lru_cache(maxsize=None)
def frame_run(frame, pid):
    return se3.run_scene(frame_scene(frame), WALL_SEED, pid)


def far_parents(res):
    """parents beyond the mirror, both trees"""
    return sum(1 for t in res["parents"] for v in t if v >= MIRROR)


# ------------------------------------------------------------------------------------------- B: one offending triple
B_BOUND = 50.0
B_FRACTION = (2.6 / 128.5) / (0.1 * se3.extent([(-B_BOUND, B_BOUND)] * 3))      # 129 states at d = 2.6
B_STEPS = {1: (1,), 2: (1, 2), 4: (1, 4), 5: (1, 5), 64: (1, 64), 65: (1, 64, 65), 129: (1, 64, 65, 128, 129)}   # S: the s* used
B_NBODY = (1, 3, 16)
B_NOBS = (1, 63, 128, 129, 200)
B_NEAR = {0: [10.0, 5.0, -7.0], 37: [-12.0, 9.0, 14.0], -1: [3.0, -15.0, 8.0]}     # obstacle index (-1: the last) -> centre
B_DIRECTION = so3.normalise([0.61, -0.47, 0.64, 0.0])[:3]
B_SIDEWAYS = so3.normalise([0.47, 0.61, 0.0, 0.0])[:3]                                # perpendicular to the direction
B_Q0 = so3.normalise([0.21, -0.34, 0.12, 0.9])
B_Q1 = so3.normalise([-0.5, 0.4, 0.55, 0.5])
B_ROTATION_SHARE = 0.3           # of a motion's SE(3) length


def b_base(nbody, n_obs):
    near = {(n_obs - 1 if j < 0 else j): c for j, c in B_NEAR.items() if j < n_obs}
    obstacles = [(near[j], 1e-4) if j in near else ([1000.0 + 5.0 * j, 0.0, 0.0], 0.5) for j in range(n_obs)]
    return dict(bounds_xyz=[(-B_BOUND, B_BOUND)] * 3, rot_bounds=None, max_distance=3.0, goal_bias=1.0, fraction=B_FRACTION, goal_r=0.25,
                body=[(c, 0.0) for c, _ in B16[:nbody]], obstacles=obstacles, max_nodes=100, max_iterations=2), sorted(near)


@functools.lru_cache(maxsize=None)
def b_motion(S):
    """the unshifted motion of S states: from the origin with B_Q0, the SE(3) length (S - 1/2) resolutions"""
    sc, _ = b_base(1, 1)
    length = (S - 0.5) * resolution(sc)
    q_to = so3.interpolate(B_Q0, B_Q1, B_ROTATION_SHARE * length / so3.distance(B_Q0, B_Q1))
    along = length - so3.distance(B_Q0, q_to)
    return [0.0, 0.0, 0.0] + B_Q0, [along * v for v in B_DIRECTION] + q_to


@functools.lru_cache(maxsize=None)
def b_batch(nbody, n_obs):
    """(scene with one start and one target per problem, problems): every (S, s*, b*, j*) of the grid as an offender -- sphere b*
    at state s* sits on obstacle j* -- and as its control, a further 0.01 sideways"""
    sc, near = b_base(nbody, n_obs)
    problems, starts, targets = [], [], []
    for S, picks in B_STEPS.items():
        frm, to = b_motion(S)
        states = motion_states(sc, frm, to)
        for s in picks:
            for b in sorted({0, nbody - 1}):
                at = se3.body_centre(states[s - 1], sc["body"][b][0])
                for j in near:
                    for control in (False, True):
                        shift = [sc["obstacles"][j][0][k] - at[k] + (0.01 * B_SIDEWAYS[k] if control else 0.0) for k in range(3)]
                        problems.append(dict(S=S, s=s, b=b, j=j, control=control))
                        starts.append([frm[k] + shift[k] for k in range(3)] + frm[3:])
                        targets.append([to[k] + shift[k] for k in range(3)] + to[3:])
    return dict(sc, start=starts, target=targets), problems


@functools.lru_cache(maxsize=None)
def b_expected(nbody, n_obs):
    """per problem: (the checker's run of two iterations, the checker's check_motion of start -> target)"""
    sc, problems = b_batch(nbody, n_obs)
    body = se3.make_body(sc)
    return [(se3.run_scene(problem_scene(sc, p), 0, p, body=body),
             se3.check_motion(body, sc["bounds_xyz"], sc["fraction"], sc["start"][p], sc["target"][p])) for p in range(len(problems))]


# ------------------------------------------------------------------------------------------- C: contact, unusual radii
C_EPS = (0.0, 2.0 ** -52, -2.0 ** -52, 2.0 ** -45, -2.0 ** -45, 2.0 ** -42, 2.0 ** -41, 2.0 ** -40, 2.0 ** -39, 2.0 ** -30)
C_PLACES = ((1, 0), (64, 0), (64, 31), (64, 63), (130, 65), (130, 129))     # (obstacles, index of the near one)
C_BODY = [([0.0, 0.0, 0.0], 0.25), ([0.5, 0.0, 0.0], 0.25)]
C_BODY0 = [(c, 0.0) for c, _ in C_BODY]
IDENTITY, HALF_TURN_Z = [0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 1.0, 0.0]
# pose: (state, the body sphere nearest to +x, where it is in the world).  The half turn puts the sphere at body (0.5, 0, 0) behind
# the one at the origin.  Around x = 1 .. 2.25 an obstacle's centre resolves 0.75 eps down to 2^-51 or 2^-52 only; the third pose
# brings the touching sphere to x = 0, where 0.75 (1 +- 2^-52) is a centre of its own: contact to the ulp.
C_POSES = {"front": ([1.0, 2.0, 3.0] + IDENTITY, 1, [1.5, 2.0, 3.0]), "turned": ([1.0, 2.0, 3.0] + HALF_TURN_Z, 0, [1.0, 2.0, 3.0]),
           "zero": ([-0.5, 2.0, 3.0] + IDENTITY, 1, [0.0, 2.0, 3.0])}
C_LONG = 6.5625                  # 70 states at the resolution of C's bounds; dyadic, so that the last state is `to` bit for bit
INF, NAN = math.inf, math.nan


def c_scene(body, n_obs, index, centre, radius, state):
    """one near obstacle (centre, radius) at `index` of n_obs, the others beyond x = 1000; problem 0 reaches `state` by a one-state
    motion, problem 1 by a 70-state motion along x"""
    obstacles = [(list(centre), radius) if j == index else ([1000.0 + 3.0 * j, 0.0, 0.0], 0.5) for j in range(n_obs)]
    starts = [[state[0] - d] + state[1:] for d in (0.0625, C_LONG)]
    return dict(bounds_xyz=[(-5.0, 5.0)] * 3, rot_bounds=None, max_distance=7.0, goal_bias=1.0, fraction=0.05, goal_r=0.25, body=body,
                obstacles=obstacles, start=starts, target=[list(state), list(state)], max_nodes=100, max_iterations=2)


def c_contact_cases(place):
    """the eps sweep: an obstacle of radius 0.5 along +x, its centre 0.75 (1 + eps) from the touching body sphere's"""
    n_obs, index = place
    for pose, (state, _, at) in C_POSES.items():
        for eps in C_EPS:
            yield "%s eps %+.3g" % (pose, eps), c_scene(C_BODY, n_obs, index, [at[0] + 0.75 * (1.0 + eps), at[1], at[2]], 0.5, state)


def c_radius_cases(place):
    n_obs, index = place
    state, _, at = C_POSES["front"]
    ahead = [at[0] + 0.75, at[1], at[2]]
    for name, body, centre, radius in (
            ("sum 0, d2 0", C_BODY, at, -0.25), ("sum 0, d2 > 0", C_BODY, ahead, -0.25), ("sum < 0, d2 0", C_BODY, at, -1.0),
            ("sum < 0, d2 > 0", C_BODY, ahead, -1.0), ("-inf, d2 0", C_BODY, at, -INF), ("-inf", C_BODY, ahead, -INF),
            ("+inf", C_BODY, ahead, INF), ("+inf far", C_BODY, [900.0, 0.0, 0.0], INF), ("nan", C_BODY, ahead, NAN),
            ("nan, d2 0", C_BODY, at, NAN), ("nan far", C_BODY, [900.0, 0.0, 0.0], NAN),
            ("point on point", C_BODY0, at, 0.0), ("point near point", C_BODY0, [at[0] + 2.0 ** -40, at[1], at[2]], 0.0),
            ("point at contact", C_BODY0, [at[0] + 0.5, at[1], at[2]], 0.5),
            ("point inside the band", C_BODY0, [at[0] + 0.5 * (1.0 + 2.0 ** -41), at[1], at[2]], 0.5),
            ("point outside the band", C_BODY0, [at[0] + 0.5 * (1.0 + 2.0 ** -39), at[1], at[2]], 0.5),
            ("point an ulp inside", C_BODY0, [at[0] + 0.5 - 2.0 ** -52, at[1], at[2]], 0.5)):
        yield name, c_scene(body, n_obs, index, centre, radius, state)


def c_expected(sc):
    """the checker's verdicts: is_valid(state), check_motion of both motions, the two planner runs"""
    body = se3.make_body(sc)
    state = sc["target"][0]
    return dict(valid=body.is_valid(state),
                motions=[se3.check_motion(body, sc["bounds_xyz"], sc["fraction"], a, state) for a in sc["start"]],
                runs=[se3.run_scene(problem_scene(sc, p), 0, p, body=body) for p in range(2)])
