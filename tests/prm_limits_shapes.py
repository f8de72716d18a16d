"""Scenes for PRM roadmap construction (prm_kernels.hip over R^n, prm_so3.hip over SO(3)) at the limits the golden scenes and the
large random roadmaps do not reach, and what each scene is expected to hold.
  rn       R^1 .. R^8, 1,300 milestones among spheres (R^1: blocked intervals), by radius and by the 8 nearest
  grid     samples on a 16 x 16 grid far from the origin: exact ties and zero distances for the k-nearest rule, screen on and off
  beyond   k larger than the roadmap (every row takes every earlier milestone), and a k-nearest search whose candidates overflow
           the pair search's first buffer
  cuts     max_samples one below, at and one above the sample that fills the roadmap, in R^2 and on SO(3)
  cones    SO(3) with 64, 65 and 130 forbidden cones: the last size that fits the edge kernel's LDS table and the first two beyond it
  bands    SO(3) radii one ulp either side of chosen pair distances, from the smallest through the LERP / SLERP switch to PI / 2

Constructions only: nothing here loads the GPU library.  R^n expectations are the C oracle's (oracle/prm_oracle.c).  The SO(3)
checker (tests/golden/make_golden_prm_so3.py) evaluates one pair at a time in Python, minutes at these sizes, so `so3_roadmap` below
restates its loop over whole arrays: the same operations in the same order on numpy's binary64, which rounds every one of them as
Python's float does.  tests/test_prm_limits_model.py holds it to the checker bit for bit -- each function on random and edge
inputs, whole roadmaps on small scenes -- and holds every scene to the property it was made for.  Oracle runs and roadmaps are
computed once (functools caches) and shared: never modify one."""
import functools
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden as mg  # noqa: E402
import make_golden_prm_so3 as gp  # noqa: E402
import make_golden_so3 as g3  # noqa: E402
from make_golden_disc import C1, C2, C3, C4, C5, C6, S1, S2, S3, S4, S5, S6  # noqa: E402

from prm_helpers import make_oracle_prm  # noqa: E402

FRACTION = 0.05
N = 1300                         # crosses the pair search's j-block of 1,024, five i-chunks of 256, no multiple of 2, 4 or 64
PAIR_JB, PAIR_IC = 1024, 256     # kPairJB, kPairIC (prm_kernels.hip, prm_so3.hip)
FIRST_CAND_BUFFER = 1 << 20      # find_pairs (oxhip_prm_api.hip): max(2^20, 64 * max_milestones) pairs
SO3_LDS_CONES = 64               # kSo3LdsCones (prm_so3.hip)
BIG = 10 ** 9


# ============================================================================================================ R^n: the oracle
def rn_params(dim, bounds, radius, seed, stream, n, spheres=(), boxes=(), max_samples=BIG, knn_k=0):
    return dict(dim=dim, bounds=[(float(lo), float(hi)) for lo, hi in bounds], radius=float(radius), fraction=FRACTION, seed=seed,
                stream=stream, max_milestones=n, max_samples=max_samples, spheres=list(spheres), boxes=list(boxes), knn_k=knn_k)


def _freeze(P):
    return (P["dim"], tuple(P["bounds"]), P["radius"], P["seed"], P["stream"], P["max_milestones"], P["max_samples"], P["knn_k"],
            tuple((tuple(c), r) for c, r in P["spheres"]), tuple((tuple(lo), tuple(hi)) for lo, hi in P["boxes"]))


_ORACLES = {}


def oracle_roadmap(P):
    """the oracle's roadmap of P, built once: dict(o, states, offsets, nbrs, n, n_samples); the query is set by `query_of`.
    Every call has a finite max_samples: on a scene where no sample is valid the oracle would not return."""
    key = _freeze(P)
    if key not in _ORACLES:
        o = make_oracle_prm(P)
        d = P["dim"]
        o.setup([0.0] * d, [0.0] * d, 0.0)
        o.construct_roadmap(P["max_milestones"], min(P["max_samples"], 4096 * P["max_milestones"]))
        states, offsets, nbrs = o.roadmap()
        for a in (states, offsets, nbrs):
            a.setflags(write=False)
        _ORACLES[key] = dict(o=o, states=states, offsets=offsets, nbrs=nbrs, n=o.num_milestones, n_samples=o.num_samples)
    return _ORACLES[key]


def query_of(P):
    """one query per scene: from the first milestone to a ball about the last one (a valid start by construction)"""
    R = oracle_roadmap(P)
    if R["n"] == 0:
        d = P["dim"]
        return [0.0] * d, [0.0] * d, 0.0
    r = P["radius"] if math.isfinite(P["radius"]) and P["radius"] > 0.0 else 1.0
    return [float(v) for v in R["states"][0]], [float(v) for v in R["states"][-1]], 0.5 * r


def pair_d2(states):
    """[n][n] squared distances as rvss.rs:137-155 sums them (sequentially over the coordinates), row j = distance(m_j, m_i)^2"""
    acc = None
    for k in range(states.shape[1]):
        d = states[:, None, k] - states[None, :, k]
        acc = d * d if acc is None else acc + d * d
    return acc


def earlier(n):
    """[n][n] mask of the pairs (j, i) with i < j"""
    return np.tri(n, n, -1, dtype=bool)


def radius_candidates(P):
    """pairs (j, i < j) with distance < radius, counted from the oracle's milestones alone"""
    st = oracle_roadmap(P)["states"]
    return int(((np.sqrt(pair_d2(st)) < P["radius"]) & earlier(len(st))).sum())


def knn_candidates(P):
    n = oracle_roadmap(P)["n"]
    return sum(min(P["knn_k"], j) for j in range(n))


# ---- 1. every dimension
# connection radius and sphere radius per dimension, chosen on the CPU with the oracle (test_prm_limits_model.py holds the choice:
# mean degree within 4 .. 40 under either rule, and motions refused by the obstacles)
RN_RADIUS = {1: 0.1, 2: 0.55, 3: 1.2, 4: 2.0, 5: 2.8, 6: 3.6, 7: 4.4, 8: 5.0}
RN_SPHERE_R = {2: (0.15, 0.5), 3: (0.4, 1.0), 4: (1.0, 2.2), 5: (1.5, 3.0), 6: (2.0, 3.6), 7: (2.5, 4.2), 8: (3.0, 4.8)}
R1_INTERVALS = [(1.5, 0.01), (3.0, 0.03), (5.25, 0.004), (7.0, 0.04), (8.75, 0.3)]   # (centre, half width): a sphere in R^1
DIMS = tuple(range(1, 9))
RN_KNN = 8


@functools.lru_cache(maxsize=None)
def rn_scene(dim, knn_k=0):
    if dim == 1:
        spheres = [([c], r) for c, r in R1_INTERVALS]
    else:
        rng = np.random.default_rng(500 + dim)
        lo, hi = RN_SPHERE_R[dim]
        count = 40 if dim <= 3 else 14
        centres = rng.uniform(0.5, 9.5, size=(count, dim))
        radii = rng.uniform(lo, hi, size=count)
        spheres = [([float(v) for v in c], float(r)) for c, r in zip(centres, radii)]
    return rn_params(dim, [(0.0, 10.0)] * dim, RN_RADIUS[dim], 40 + dim, dim, N, spheres=spheres, knn_k=knn_k)


def r1_pairs_across(P):
    """R^1: pairs of milestones on either side of a blocked interval and closer than the radius, per interval"""
    x = np.sort(oracle_roadmap(P)["states"][:, 0])
    out = []
    for (c,), r in P["spheres"]:
        left, right = x[x < c - r], x[x > c + r]
        out.append(int(((right[None, :] - left[:, None]) < P["radius"]).sum()) if len(left) and len(right) else 0)
    return out


# ---- 2. ties on a coarse grid
GRID_KS = (1, 8, 33)
GRID_FRAMES = {"screen_on": (2.0 ** 49, 2.0), "screen_off": (2.0 ** 51, 8.0)}   # offset (below / above 1e15), width: 16 values per axis


@functools.lru_cache(maxsize=None)
def grid_scene(frame, knn_k):
    z0, w = GRID_FRAMES[frame]
    return rn_params(2, [(z0, z0 + w)] * 2, 0.25 * w, 7, 1, N, knn_k=knn_k)


def knn_row_thresholds(P, n_now, n_samples, rounds=None):
    """knn_row_radii (oxhip_prm_api.hip) restated: row j > 6 k searches the squared radius expected to hold 6 k earlier milestones;
    the rows up to 6 k take every earlier milestone (+inf).  `rounds`: (n_done, n_now, n_samples) of every round of a roadmap built
    under a wall clock (each round estimates the valid fraction of the box from its own counts); default: one round"""
    dim, k = P["dim"], P["knn_k"]
    vol = 1.0
    for lo, hi in P["bounds"]:
        vol *= hi - lo
    c_d = math.pow(3.14159265358979323846, 0.5 * dim) / math.gamma(0.5 * dim + 1.0)
    want = 6.0 * k
    thr = np.full(n_now, np.inf)
    for first, last, samples in rounds or [(0, n_now, n_samples)]:
        frac = min(1.0, float(last) / float(samples)) if samples else 1.0
        for j in range(first, last):
            if float(j) <= want:
                continue
            r = math.pow(want * vol * frac / (c_d * float(j)), 1.0 / dim)
            thr[j] = r * r
    return thr


def knn_search_hits(states, thr):
    """per row j: the earlier milestones with d2 <= thr[j], what the pair search hands the selection"""
    hits = np.zeros(len(states), dtype=np.int64)
    for j0 in range(0, len(states), 500):
        d2 = None
        for k in range(states.shape[1]):
            d = states[j0:j0 + 500, None, k] - states[None, :, k]
            d2 = d * d if d2 is None else d2 + d * d
        rows = np.arange(j0, min(j0 + 500, len(states)))
        hits[rows] = ((d2 <= thr[rows, None]) & (np.arange(len(states))[None, :] < rows[:, None])).sum(axis=1)
    return hits


_KNN_MODELS = {}


def knn_model(P):
    """what the k-nearest search meets on scene P: tie rows (the k-th and (k+1)-th nearest earlier milestones at exactly equal
    distance), zero distances, the rows whose candidate radius holds fewer than min(k, j) earlier milestones (they take the exact
    search), all candidates of the radius search, and how close any squared distance comes to its row's threshold"""
    key = _freeze(P)
    if key not in _KNN_MODELS:
        _KNN_MODELS[key] = _knn_model(P)
    return _KNN_MODELS[key]


def _knn_model(P):
    R = oracle_roadmap(P)
    st, n, k = R["states"], R["n"], P["knn_k"]
    d2 = pair_d2(st)
    before = earlier(n)
    thr = knn_row_thresholds(P, n, R["n_samples"])
    hits = knn_search_hits(st, thr)
    need = np.minimum(k, np.arange(n))
    d = np.where(before, np.sqrt(d2), np.inf)
    d.sort(axis=1)
    rows = np.arange(n) > k
    ties = int((rows & (d[:, k - 1] == d[:, min(k, n - 1)])).sum()) if n > k else 0
    finite = np.isfinite(thr)
    rel = np.abs(d2[finite] - thr[finite, None]) / thr[finite, None]
    return dict(tie_rows=ties, zero_pairs=int(((d2 == 0.0) & before).sum()), radius_rows=int(finite.sum()),
                short_rows=int((hits < need).sum()), full_rows=int(((hits >= need) & finite).sum()), candidates=int(hits.sum()),
                closest_to_threshold=float(rel.min()) if finite.any() else math.inf, distinct=len({tuple(r) for r in st.tolist()}))


# ---- 3. k beyond the roadmap, and the k-nearest search through the candidate overflow
BEYOND_K, BEYOND_N = 2000, 300
OVERFLOW_N = 3000
OVERFLOW_K = 120                 # 80 brings 803,206 candidates, 100 brings 971,779: short of the buffer (the box cuts the balls)


def _r3_spheres():
    rng = np.random.default_rng(77)
    return [([float(v) for v in c], float(r)) for c, r in zip(rng.uniform(1.0, 9.0, size=(10, 3)), rng.uniform(0.5, 1.4, size=10))]


@functools.lru_cache(maxsize=None)
def beyond_scene(rule):
    """rule "knn": the 2,000 nearest of at most 299 earlier milestones; rule "radius": radius +inf -- the same roadmap"""
    if rule == "knn":
        return rn_params(3, [(0.0, 10.0)] * 3, 1.5, 31, 4, BEYOND_N, spheres=_r3_spheres(), knn_k=BEYOND_K)
    return rn_params(3, [(0.0, 10.0)] * 3, math.inf, 31, 4, BEYOND_N, spheres=_r3_spheres())


@functools.lru_cache(maxsize=None)
def overflow_scene():
    return rn_params(3, [(0.0, 10.0)] * 3, 1.5, 32, 6, OVERFLOW_N, spheres=_r3_spheres(), knn_k=OVERFLOW_K)


# ---- 4. where a round ends (R^2 with a box; the SO(3) twin is `so3_cut_scene` below)
CUT_N = 600


@functools.lru_cache(maxsize=None)
def rn_cut_scene(max_samples=BIG):
    return rn_params(2, [(0.0, 10.0)] * 2, 0.6, 19, 2, CUT_N, boxes=[([3.0, 0.0], [6.5, 7.0])], spheres=[([8.0, 8.5], 0.8)],
                     max_samples=max_samples)


def rn_fill_samples():
    """S: the sample that fills the roadmap"""
    return oracle_roadmap(rn_cut_scene())["n_samples"]


# ========================================================================================= SO(3): the checker over whole arrays
def _hi(x):
    return (np.ascontiguousarray(x, dtype=np.float64).view(np.uint64) >> np.uint64(32)).astype(np.int64)


def _from_hi(h):
    return (h.astype(np.uint64) << np.uint64(32)).view(np.float64)


def _acos_r(z):
    p = z * (g3.PS0 + z * (g3.PS1 + z * (g3.PS2 + z * (g3.PS3 + z * (g3.PS4 + z * g3.PS5)))))
    q = 1.0 + z * (g3.QS1 + z * (g3.QS2 + z * (g3.QS3 + z * g3.QS4)))
    return p / q


def ox_acos(x):
    """make_golden_so3.ox_acos on an array of values in [0, 1] (what |dot| and a sign-corrected dot are; beyond 1: NaN)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    assert not (x < 0.0).any()
    ix = _hi(x) & 0x7FFFFFFF
    with np.errstate(invalid="ignore", divide="ignore"):
        zs = x * x
        small = g3.PIO2_HI - (x - (g3.PIO2_LO - x * _acos_r(zs)))
        small = np.where(ix <= 0x3C600000, g3.PIO2_HI + g3.PIO2_LO, small)
        z = (1.0 - x) * 0.5
        s = np.sqrt(z)
        df = _from_hi(_hi(s))
        c = (z - df * df) / (s + df)
        big = 2.0 * (df + (_acos_r(z) * s + c))
    out = np.where(ix < 0x3FE00000, small, big)
    out = np.where(ix >= 0x3FF00000, np.where(x == 1.0, 0.0, np.nan), out)
    return out


def _k_sin0(x):
    z = x * x
    v = z * x
    r = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)))
    return x + v * (S1 + z * r)


def _k_cos(x, y):
    ix = _hi(x) & 0x7FFFFFFF
    z = x * x
    r = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))))
    qx = np.where(ix > 0x3FE90000, 0.28125, _from_hi(np.maximum(ix - 0x00200000, 0)))
    hz = 0.5 * z - qx
    a = 1.0 - qx
    return np.where(ix < 0x3FD33333, 1.0 - (0.5 * z - (z * r - x * y)), a - (hz - (z * r - x * y)))


def ox_sin(x):
    """make_golden_disc.ox_sincos(x)[0] on an array of values in [0, 3 PI / 4): the angles SO(3) interpolation takes a sine of"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    pio2_1, pio2_1t = 1.57079632673412561417e+00, 6.07710050650619224932e-11
    pio2_2, pio2_2t = 6.07710050630396597660e-11, 2.02226624879595063154e-21
    pio2_3, pio2_3t = 2.02226624871116645580e-21, 8.47842766036889956997e-32
    ix = _hi(x) & 0x7FFFFFFF
    assert not (x < 0.0).any() and not (x >= 2.35).any()      # n = int(x * invpio2 + 0.5) is 0 or 1
    direct = np.where(ix < 0x3E400000, x, _k_sin0(x))
    # n = 1: sin x = cos(x - PI / 2), the argument reduced in up to three steps
    r = x - pio2_1
    w = np.full_like(x, pio2_1t)
    j = ix >> 20
    y0 = r - w
    i = j - ((_hi(y0) >> 20) & 0x7FF)
    second = i > 16
    t = r
    w2 = np.full_like(x, pio2_2)
    r2 = t - w2
    w2 = pio2_2t - ((t - r2) - w2)
    y02 = r2 - w2
    i2 = j - ((_hi(y02) >> 20) & 0x7FF)
    third = second & (i2 > 49)
    t3 = r2
    w3 = np.full_like(x, pio2_3)
    r3 = t3 - w3
    w3 = pio2_3t - ((t3 - r3) - w3)
    y03 = r3 - w3
    r = np.where(third, r3, np.where(second, r2, r))
    w = np.where(third, w3, np.where(second, w2, w))
    y0 = np.where(third, y03, np.where(second, y02, y0))
    y1 = (r - y0) - w
    return np.where(ix <= 0x3FE921FB, direct, _k_cos(y0, y1))


def so3_dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2] + a[..., 3] * b[..., 3]


def so3_distance(a, b):
    ad = np.abs(so3_dot(a, b))
    far = ad <= 1.0 - 1e-9
    out = np.zeros(ad.shape)
    out[far] = ox_acos(ad[far])
    return out


class So3Motions:
    """make_golden_so3.interpolate for [m] motions (frm, to [m][4]) at t [m].  What does not depend on t -- the sign, the branch,
    theta and its sine -- is computed when the motions are given and not again at every t: the same values"""

    def __init__(self, frm, to):
        self.frm, self.to = frm, to
        d = so3_dot(frm, to)
        self.sign = np.where(d < 0.0, -1.0, 1.0)
        d = d * self.sign
        self.slerp = ~(d > 0.9995)
        self.theta = ox_acos(d[self.slerp])
        self.sin_theta = ox_sin(self.theta)

    def at(self, t, rows=None):
        """the states at t; `rows`: of these motions only (t is then theirs)"""
        rows = np.arange(len(self.frm)) if rows is None else rows
        frm, to, sign = self.frm[rows], self.to[rows], self.sign[rows]
        o = frm + t[:, None] * (to * sign[:, None] - frm)
        norm = np.sqrt(o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1] + o[:, 2] * o[:, 2] + o[:, 3] * o[:, 3])
        out = o / norm[:, None]
        sl = self.slerp[rows]
        if sl.any():
            pos = np.cumsum(self.slerp) - 1                 # a motion's place among the SLERP ones
            k = pos[rows[sl]]
            theta, sin_theta, ts = self.theta[k], self.sin_theta[k], t[sl]
            s0 = ox_sin((1.0 - ts) * theta) / sin_theta
            s1 = ox_sin(ts * theta) / sin_theta * sign[sl]
            out[sl] = frm[sl] * s0[:, None] + to[sl] * s1[:, None]
        return out


def so3_interpolate(frm, to, t):
    return So3Motions(frm, to).at(t)


class ConeField:
    """make_golden_so3.Cones over arrays: valid iff distance(centre, q) > radius for every cone.  A cone is settled by a rounded
    matrix product where |dot| is further than 1e-6 from cos(radius) -- acos falls at least as fast as its argument rises and
    ox_acos is within 2^-50 of it (tests/test_prm_so3_oracle_golden.py), the product within 1e-15 -- and by the checker's own
    distance everywhere else"""
    MARGIN = 1e-6

    def __init__(self, cones):
        self.c = np.array([c for c, _ in cones], dtype=np.float64).reshape(-1, 4)
        self.r = np.array([r for _, r in cones], dtype=np.float64)
        cr = np.cos(np.clip(self.r, 0.0, None))
        # a radius beyond PI / 2 or below 0, or a NaN, is never settled by the product
        plain = (self.r >= 0.0) & (self.r <= 1.5)
        self.hi = np.where(plain, cr + self.MARGIN, np.inf)
        self.lo = np.where(plain, cr - self.MARGIN, -np.inf)

    def is_valid(self, q):
        q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 4)
        if len(self.r) == 0:
            return np.ones(len(q), dtype=bool)
        a = np.abs(q @ self.c.T)
        bad = (a > self.hi).any(axis=1)
        rows, cones = np.nonzero((a >= self.lo) & (a <= self.hi) & ~bad[:, None])
        if len(rows):
            inside = ~(so3_distance(self.c[cones], q[rows]) > self.r[cones])
            bad[rows[inside]] = True
        return ~bad


def so3_motion_valid(field, fraction, frm, to):
    """make_golden_so3.check_motion for [m] motions at once"""
    seg = g3.lvsl(fraction) * 0.1
    q = so3_distance(frm, to) / seg
    n = np.ceil(q)                                    # mg.num_steps: the distances are finite and not negative
    ok = np.ones(len(frm), dtype=bool)
    short = n <= 1.0
    if short.any():
        ok[short] = field.is_valid(to[short])
    live = np.nonzero(~short)[0]
    motions = So3Motions(frm, to)
    i = 1.0
    while len(live):
        t = i / n[live]
        good = field.is_valid(motions.at(t, live))
        ok[live[~good]] = False
        live = live[good & (n[live] > i)]
        i += 1.0
    return ok


def _so3_key(sc):
    return (None if sc["bounds"] is None else (tuple(sc["bounds"][0]), sc["bounds"][1]), sc["fraction"], sc["seed"], sc["stream"],
            tuple((tuple(c), r) for c, r in sc["cones"]))


_SO3_SAMPLES, _SO3_PAIRS = {}, {}


def so3_milestones(sc, n, max_samples=BIG):
    """the first n milestones of the scene's stream and the sample_uniform calls made when the n-th arrives (prm_construct's
    sampling: the milestones do not depend on the roadmap), cut at max_samples calls"""
    key = _so3_key(sc)
    if key not in _SO3_SAMPLES:
        _SO3_SAMPLES[key] = dict(rng=mg.ChaCha12Rng(sc["seed"], sc["stream"]), states=[], calls_at=[], calls=0,
                                 field=ConeField(sc["cones"]), frame=g3.space_bounds(sc["bounds"]))
    S = _SO3_SAMPLES[key]
    while len(S["states"]) < n and S["calls"] < 4096 * n:
        q = g3.sample_uniform(S["rng"], *S["frame"])
        S["calls"] += 1
        if S["field"].is_valid(q)[0]:
            S["states"].append(q)
            S["calls_at"].append(S["calls"])
    assert len(S["states"]) >= n
    if max_samples >= S["calls_at"][n - 1]:
        return np.array(S["states"][:n]).reshape(-1, 4), S["calls_at"][n - 1]
    m = int(np.searchsorted(S["calls_at"], max_samples, side="right"))
    return np.array(S["states"][:m]).reshape(-1, 4), max_samples


def so3_pairs(sc, n):
    """every pair (j, i < j) of the first n milestones: its distance and (filled on demand by `so3_roadmap`) whether
    check_motion(m_j -> m_i) holds -- neither depends on the connection radius"""
    key = (_so3_key(sc), n)
    if key not in _SO3_PAIRS:
        st, _ = so3_milestones(sc, n)
        jj, ii = np.nonzero(earlier(n))
        _SO3_PAIRS[key] = dict(j=jj, i=ii, d=so3_distance(st[jj], st[ii]), motion=np.zeros(len(jj), dtype=np.int8))   # 0: not checked yet
    return _SO3_PAIRS[key]


def so3_roadmap(sc, radius=None, n=None, max_samples=None):
    """gp.prm_construct(sc) with the loops over arrays: dict(states [n][4], edges (a list per node, ascending), n_samples,
    candidates (pairs with distance < radius))"""
    radius = sc["radius"] if radius is None else radius
    n_full = sc["max_milestones"] if n is None else n
    st, calls = so3_milestones(sc, n_full, sc["max_samples"] if max_samples is None else max_samples)
    n_now = len(st)
    P = so3_pairs(sc, n_full)
    cand = np.nonzero((P["d"] < radius) & (P["j"] < n_now))[0]
    todo = cand[P["motion"][cand] == 0]
    if len(todo):
        full, _ = so3_milestones(sc, n_full)
        ok = so3_motion_valid(_SO3_SAMPLES[_so3_key(sc)]["field"], sc["fraction"], full[P["j"][todo]], full[P["i"][todo]])
        P["motion"][todo] = np.where(ok, 1, -1)
    keep = cand[P["motion"][cand] == 1]
    u = np.concatenate([P["j"][keep], P["i"][keep]])
    v = np.concatenate([P["i"][keep], P["j"][keep]])
    order = np.lexsort((v, u))
    u, v = u[order], v[order]
    cuts = np.searchsorted(u, np.arange(n_now + 1))
    edges = [[int(x) for x in v[cuts[k]:cuts[k + 1]]] for k in range(n_now)]
    return dict(states=st, edges=edges, n_samples=calls, candidates=len(cand), valid_candidates=len(keep))


# ---- 4. where a round ends, SO(3)
def so3_cut_scene():
    return dict(gp.scenes()["bounded"], max_milestones=CUT_N)


def so3_fill_samples():
    return so3_milestones(so3_cut_scene(), CUT_N)[1]


# ---- 5. the cone table beyond LDS, and the |dot| bands
CONE_COUNTS = (64, 65, 130)
CONE_RADIUS = 0.4


@functools.lru_cache(maxsize=None)
def cones_scene(count):
    rng = np.random.default_rng(900 + count)
    centres = rng.normal(size=(count, 4))
    cones = [(g3.normalise([float(v) for v in c]), float(r)) for c, r in zip(centres, rng.uniform(0.02, 0.12, size=count))]
    fx = gp.fixture_scene()
    return dict(fx, cones=cones, radius=CONE_RADIUS, seed=13, stream=count, max_milestones=N)


BAND_N = 400
BAND_TARGETS = ("smallest", 0.0316, 0.3, 1.0, "largest")
BAND_CUTOFF_RADII = (1e-6, 4.5e-5)      # either side of acos(1 - 1e-9) = 4.47e-5, below which the distance is 0 by definition


def bands_scene():
    return dict(gp.scenes()["fixture"], max_milestones=BAND_N)


@functools.lru_cache(maxsize=None)
def band_pairs():
    """target -> (j, i, d): the pair of the scene whose distance is nearest the target (the smallest one: non-zero)"""
    P = so3_pairs(bands_scene(), BAND_N)
    d = P["d"]
    out = {}
    for target in BAND_TARGETS:
        if target == "smallest":
            k = int(np.argmin(np.where(d > 0.0, d, np.inf)))
        elif target == "largest":
            k = int(np.argmax(d))
        else:
            k = int(np.argmin(np.abs(d - target)))
        out[target] = (int(P["j"][k]), int(P["i"][k]), float(d[k]))
    return out


def band_radii(d):
    return (math.nextafter(d, 0.0), d, math.nextafter(d, math.inf))


def so3_radius_bands(r):
    """so3_radius_bands (oxhip_prm_api.hip): |dot| above hi is inside the radius, below lo outside, in between ox_acos decides"""
    if not (r <= g3.PIO2_HI):
        return -1.0, -1.0
    hi = math.cos(r * (1.0 - 2.0 ** -40)) + 2.0 ** -50
    lo = min(math.cos(r * (1.0 + 2.0 ** -40)) - 2.0 ** -50, 1.0 - 1e-9)
    return lo, hi
