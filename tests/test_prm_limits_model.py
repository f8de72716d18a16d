"""CPU: every scene of tests/prm_limits_shapes.py has the property tests/test_gpu_prm_limits.py needs it for, shown from the C oracle
(oracle/prm_oracle.c), the SO(3) checker (tests/golden/make_golden_prm_so3.py) and a restatement of the host's k-nearest candidate
radii alone; and the array form of the SO(3) checker that the shapes module uses at 1,300 milestones is the checker bit for bit --
function by function on random and edge inputs, and as whole roadmaps.  The GPU test compares the device with these references bit
for bit, so what holds of the input here holds of the device's run.  The counts are printed: the run's output is the record."""
import math
import random

import numpy as np
import pytest

import prm_limits_shapes as shapes
from helpers import bits
from make_golden_disc import ox_sincos
from prm_limits_shapes import g3, gp


def _same_bits(a, b):
    return np.array_equal(bits(np.asarray(a, dtype=np.float64)), bits(np.asarray(b, dtype=np.float64)))


# ------------------------------------------------------------------------------------------- the array form of the SO(3) checker
def test_array_acos_and_sin_are_the_checkers():
    rnd = np.random.default_rng(1)
    xs = np.concatenate([rnd.random(20000), 1.0 - 10.0 ** -rnd.uniform(1, 12, 20000), rnd.random(5000) * 1e-3,
                         [0.0, 0.5, 1.0, 1.0 - 1e-9, 2.0 ** -56, 2.0 ** -30, math.nextafter(0.5, 0.0), math.nextafter(1.0, 0.0), 0.9995]])
    assert _same_bits(shapes.ox_acos(xs), [g3.ox_acos(float(x)) for x in xs])
    half = math.pi / 2
    ys = np.concatenate([rnd.random(30000) * 2.3, rnd.random(5000) * 1e-7, half + (rnd.random(5000) - 0.5) * 1e-6,
                         half + (rnd.random(5000) - 0.5) * 1e-13,      # the second and third reduction steps
                         [0.0, half, math.pi / 4, math.nextafter(half, 0.0), math.nextafter(half, 4.0), 0.7853981633974483,
                          0.7853981633974484, 0.785398163397448, 2.0 ** -27, 2.0 ** -26]])
    assert _same_bits(shapes.ox_sin(ys), [ox_sincos(float(y))[0] for y in ys])


def _random_rotations(rnd, n):
    return np.array([g3.normalise([rnd.gauss(0.0, 1.0) for _ in range(4)]) for _ in range(n)])


def test_array_distance_interpolation_and_motion_check_are_the_checkers():
    rnd = random.Random(3)
    a = _random_rotations(rnd, 600)
    b = _random_rotations(rnd, 600)
    # close pairs either side of the LERP / SLERP switch and of the 1 - 1e-9 cut, and their antipodal copies
    for k, eps in enumerate([0.0, 1e-12, 1e-6, 4.4e-5, 4.6e-5, 1e-3, 0.0316, 0.0317, 0.03] * 20):
        b[k] = g3.normalise([a[k][0] + eps * rnd.gauss(0, 1), a[k][1] + eps, a[k][2] - eps * rnd.random(), a[k][3]])
    b[100:200] = -b[100:200]
    want = [g3.distance(list(p), list(q)) for p, q in zip(a, b)]
    assert _same_bits(shapes.so3_distance(a, b), want)
    assert sum(1 for d in want if d == 0.0) >= 20 and sum(1 for d in want if 0.0 < d < 0.0316) >= 20
    t = np.array([rnd.choice([0.0, 1.0, 0.5, rnd.random()]) for _ in range(600)])
    assert _same_bits(shapes.so3_interpolate(a, b, t), [g3.interpolate(list(p), list(q), float(x)) for p, q, x in zip(a, b, t)])
    # the cone field: states on, just inside and just outside the rim of a cone, many cones; and whole motions
    sc = shapes.cones_scene(65)
    field, cones = shapes.ConeField(sc["cones"]), g3.Cones(sc["cones"])
    rim = []
    for c, r in sc["cones"][:40]:
        for dr in (0.0, 1e-15, -1e-15, 1e-9, -1e-9, 2e-6, -2e-6, 1e-3):
            axis = g3.normalise([rnd.gauss(0, 1), rnd.gauss(0, 1), rnd.gauss(0, 1), 0.0])[:3]
            step = g3.quaternion_from_axis_angle(axis, 2.0 * (r + dr))
            x1, y1, z1, w1 = c
            x2, y2, z2, w2 = step
            rim.append(g3.normalise([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                                     w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2]))
    rim = np.array(rim)
    want = [cones.is_valid(list(q)) for q in rim]
    assert list(field.is_valid(rim)) == want and 50 < sum(want) < len(want) - 50
    want = [g3.check_motion(cones, sc["fraction"], list(p), list(q)) for p, q in zip(a[:300], b[:300])]
    assert list(shapes.so3_motion_valid(field, sc["fraction"], a[:300], b[:300])) == want
    assert 20 < sum(want) < 280


@pytest.mark.parametrize("name,n,radius", [("fixture", 120, None), ("bounded", 160, None), ("wide_radius", 25, None), ("tiny_radius", 100, None),
                                           ("fixture", 45, 1.0), ("cones65", 48, 0.6), ("cones130", 60, 0.4)])
def test_array_roadmap_is_the_checkers(name, n, radius):
    sc = shapes.cones_scene(int(name[5:])) if name.startswith("cones") else gp.scenes()[name]
    radius = sc["radius"] if radius is None else radius
    full = None
    for cap in (shapes.BIG, -1, 0, 1):       # the whole roadmap, then max_samples one below, at and one above the filling sample
        max_samples = cap if full is None else full["n_samples"] + cap
        want = gp.prm_construct(sc["bounds"], radius, sc["fraction"], g3.Cones(sc["cones"]), sc["seed"], sc["stream"], n, max_samples)
        mine = shapes.so3_roadmap(sc, radius=radius, n=n, max_samples=max_samples)
        assert _same_bits(mine["states"], np.array(want["states"]).reshape(-1, 4))
        assert mine["edges"] == want["edges"] and mine["n_samples"] == want["n_samples"]
        full = full or want
        if name == "tiny_radius":
            break
    print(name, "n", n, "samples", full["n_samples"], "candidates", mine["candidates"], "of them valid", mine["valid_candidates"])


# ------------------------------------------------------------------------------------------------------ 1. every dimension
@pytest.mark.parametrize("knn_k", [0, shapes.RN_KNN])
@pytest.mark.parametrize("dim", shapes.DIMS)
def test_rn_scene_has_a_moderate_degree_and_refused_motions(dim, knn_k):
    P = shapes.rn_scene(dim, knn_k)
    R = shapes.oracle_roadmap(P)
    candidates = shapes.knn_candidates(P) if knn_k else shapes.radius_candidates(P)
    degree = len(R["nbrs"]) / R["n"]
    print("R^%d k=%d: samples %d, mean degree %.2f, candidates %d, edges %d" % (dim, knn_k, R["n_samples"], degree, candidates, len(R["nbrs"]) // 2))
    assert R["n"] == shapes.N == 1300 and R["n_samples"] > R["n"]
    # a second j-block, five i-chunks and more, no whole number of waves, and ranges of i (they end at j - 1) of odd length
    assert shapes.N > shapes.PAIR_JB and (shapes.N - 1) // shapes.PAIR_IC >= 5 and shapes.N % 64 and (shapes.N - 1) % shapes.PAIR_IC % 2 == 1
    assert 4.0 <= degree <= 40.0
    assert 2 * candidates > len(R["nbrs"]) > 0                      # check_motion refused an in-radius pair (a nearest one)
    if knn_k:
        m = shapes.knn_model(P)
        print("   k-nearest search: rows by radius %d, short %d, candidates %d" % (m["radius_rows"], m["short_rows"], m["candidates"]))
        assert m["closest_to_threshold"] > 1e-9    # the GPU test holds the device to these counts: they must not hang on pow's last bit
    if dim == 1:
        across = shapes.r1_pairs_across(P)
        print("   pairs across the blocked intervals", across)
        assert sum(1 for c in across if c >= 1) >= 3
        # no edge crosses an interval wider than a motion's step (extent * fraction / 10 = 0.05); a narrower one can be stepped over
        wide = [c for (c,), r in P["spheres"] if 2.0 * r > 0.05]
        x = R["states"][:, 0]
        stepped_over = 0
        for j in range(R["n"]):
            for i in R["nbrs"][int(R["offsets"][j]):int(R["offsets"][j + 1])]:
                lo, hi = sorted((x[j], x[int(i)]))
                assert not any(lo < c < hi for c in wide)
                stepped_over += any(lo < c < hi for (c,), _ in P["spheres"])
        print("   edge entries across a narrow interval", stepped_over)
        assert len(wide) == 3 and sum(1 for c, n in zip(P["spheres"], across) if c[0][0] in wide and n >= 1) >= 2


# ------------------------------------------------------------------------------------------------------ 2. ties on a grid
@pytest.mark.parametrize("frame", list(shapes.GRID_FRAMES))
def test_grid_scene_ties_and_short_rows(frame):
    z0, w = shapes.GRID_FRAMES[frame]
    for k in shapes.GRID_KS:
        P = shapes.grid_scene(frame, k)
        R = shapes.oracle_roadmap(P)
        m = shapes.knn_model(P)
        print("grid %s k=%d:" % (frame, k), m)
        assert R["n"] == R["n_samples"] == shapes.N                      # no obstacle: the valid fraction of knn_row_radii is 1
        assert m["tie_rows"] >= 500 and m["zero_pairs"] >= 500 and m["distinct"] <= 256
        assert m["closest_to_threshold"] > 1e-9        # the short-row count does not hang on the last bit of pow / tgamma
        if k == 1:
            assert m["short_rows"] >= 10 and m["full_rows"] >= 10
    st = shapes.oracle_roadmap(shapes.grid_scene(frame, 1))["states"]
    assert np.array_equal((st - z0) * (16.0 / w), np.round((st - z0) * (16.0 / w)))      # 16 values per axis
    if frame == "screen_on":
        assert z0 + w < 1e15 and len(np.unique(st.astype(np.float32))) == 1                  # screened, and the screen sees one point
    else:
        assert z0 > 1e15                                                                     # host_screen_threshold: +inf


def test_grid_frames_hold_the_same_graph():
    """the two frames are one grid in different units: the same ties, the same short rows, the same roadmap"""
    for k in shapes.GRID_KS:
        a, b = (shapes.oracle_roadmap(shapes.grid_scene(f, k)) for f in shapes.GRID_FRAMES)
        assert np.array_equal(a["offsets"], b["offsets"]) and np.array_equal(a["nbrs"], b["nbrs"])
        assert shapes.knn_model(shapes.grid_scene("screen_on", k)) == shapes.knn_model(shapes.grid_scene("screen_off", k))


# ------------------------------------------------------------------------------------- 3. k beyond the roadmap; the overflow
def test_k_beyond_the_roadmap_is_the_infinite_radius():
    a, b = shapes.oracle_roadmap(shapes.beyond_scene("knn")), shapes.oracle_roadmap(shapes.beyond_scene("radius"))
    assert a["n"] == b["n"] == shapes.BEYOND_N < shapes.BEYOND_K and a["n_samples"] == b["n_samples"]
    assert _same_bits(a["states"], b["states"]) and np.array_equal(a["offsets"], b["offsets"]) and np.array_equal(a["nbrs"], b["nbrs"])
    every_pair = shapes.BEYOND_N * (shapes.BEYOND_N - 1) // 2
    assert shapes.knn_candidates(shapes.beyond_scene("knn")) == every_pair
    print("k beyond the roadmap: %d pairs, %d edges" % (every_pair, len(a["nbrs"]) // 2))
    assert 0 < len(a["nbrs"]) < 2 * every_pair                      # and the obstacles refuse some of them
    assert float(shapes.BEYOND_N) <= 6.0 * shapes.BEYOND_K         # knn_row_radii: no row gets a radius


def test_knn_candidates_overflow_the_first_buffer():
    P = shapes.overflow_scene()
    m = shapes.knn_model(P)
    print("k-nearest overflow scene:", m)
    assert max(shapes.FIRST_CAND_BUFFER, 64 * P["max_milestones"]) == shapes.FIRST_CAND_BUFFER == 2 ** 20
    assert m["candidates"] > 1.05 * 2 ** 20                         # (5 %: the count must not hang on the last bit of pow)
    assert m["closest_to_threshold"] > 1e-9
    assert m["short_rows"] >= 1                                     # and rows of it go through the exact search as well


def test_recorded_two_round_knn_counters_are_the_models():
    """tests/golden/prm_host_counters.json is a record of a device run; its k-nearest config is held here to the oracle and the
    restated candidate radii of its two rounds (4,096 milestones, then 5,000).  The library that wrote the file counted 698,009
    candidates: these, and one pair for each of the 120 slots beyond the last milestone with each of the 4,999 milestones below them"""
    import json
    import os
    import make_golden_prm_host_counters as gen
    with open(os.path.join(shapes.HERE, "golden", "prm_host_counters.json")) as f:
        rec = json.load(f)["configs"]["r3_knn_two_rounds"]
    cfg = dict(gen.CONFIGS)["r3_knn_two_rounds"]
    centres, radii = cfg["spheres"]
    P = shapes.rn_params(cfg["dim"], list(zip(cfg["bounds"][0::2], cfg["bounds"][1::2])), cfg["radius"], cfg["seed"], cfg["stream"],
                         cfg["max_milestones"], spheres=list(zip(centres, radii)), knn_k=cfg["knn_k"])
    first_round = 4096                                              # construct_roadmap under a wall clock: 4,096, then doubling
    R, R1 = shapes.oracle_roadmap(P), shapes.oracle_roadmap(dict(P, max_milestones=first_round))
    n = R["n"]
    thr = shapes.knn_row_thresholds(P, n, None, rounds=[(0, first_round, R1["n_samples"]), (first_round, n, R["n_samples"])])
    hits = shapes.knn_search_hits(R["states"], thr)
    short = int((hits < np.minimum(P["knn_k"], np.arange(n))).sum())
    print("r3_knn_two_rounds: candidates", int(hits.sum()), "short rows", short)
    assert (n, len(R["nbrs"]), R["n_samples"]) == (rec["n_milestones"], rec["edge_entries"], rec["n_samples"])
    assert (int(hits.sum()), short) == (rec["n_candidates"], rec["knn_exact_rows"])
    assert int(hits.sum()) + (-n % shapes.PAIR_JB) * (n - 1) == 698009


# -------------------------------------------------------------------------------------------------- 4. where a round ends
def test_rn_cut_scene():
    S = shapes.rn_fill_samples()
    full = shapes.oracle_roadmap(shapes.rn_cut_scene())
    print("R^2 cut scene: the roadmap fills at sample", S)
    assert full["n"] == shapes.CUT_N and S > shapes.CUT_N + 100    # samples and milestones differ
    for delta, n in ((-1, shapes.CUT_N - 1), (0, shapes.CUT_N), (1, shapes.CUT_N)):
        R = shapes.oracle_roadmap(shapes.rn_cut_scene(S + delta))
        assert (R["n"], R["n_samples"]) == (n, min(S, S + delta))
        assert _same_bits(R["states"], full["states"][:n])


def test_so3_cut_scene():
    sc = shapes.so3_cut_scene()
    S = shapes.so3_fill_samples()
    attempts = shapes._SO3_SAMPLES[shapes._so3_key(sc)]["rng"].draws // 4
    print("SO(3) cut scene: the roadmap fills at sample_uniform call", S, "which is attempt", attempts)
    assert attempts > S + 100 and S > shapes.CUT_N + 10             # attempts, accepted attempts and milestones all differ
    full = shapes.so3_roadmap(sc)
    for delta, n in ((-1, shapes.CUT_N - 1), (0, shapes.CUT_N), (1, shapes.CUT_N)):
        rm = shapes.so3_roadmap(sc, max_samples=S + delta)
        assert (len(rm["states"]), rm["n_samples"]) == (n, min(S, S + delta))
        assert rm["edges"] == [[i for i in e if i < n] for e in full["edges"][:n]]
    assert len(full["edges"][shapes.CUT_N - 1]) > 0                 # the last milestone has edges: one call early loses them


# ------------------------------------------------------------------------------- 5. the cone table beyond LDS, and the bands
@pytest.mark.parametrize("count", shapes.CONE_COUNTS)
def test_cones_scene_refuses_some_motions_and_accepts_some(count):
    sc = shapes.cones_scene(count)
    rm = shapes.so3_roadmap(sc)
    print("%d cones: samples %d, candidates %d, of them valid %d" % (count, rm["n_samples"], rm["candidates"], rm["valid_candidates"]))
    assert len(sc["cones"]) == count and (count > shapes.SO3_LDS_CONES) == (count != 64)
    assert all(0.02 <= r <= 0.12 and abs(g3.dot(c, c) - 1.0) < 1e-12 for c, r in sc["cones"])
    assert len(rm["states"]) == shapes.N and rm["n_samples"] > shapes.N
    assert rm["candidates"] - 100 > rm["valid_candidates"] > 100


def test_band_targets_are_found():
    sc = shapes.bands_scene()
    P = shapes.so3_pairs(sc, shapes.BAND_N)
    zero = int((P["d"] == 0.0).sum())
    print("band scene: %d pairs, %d of them at distance exactly 0; smallest %r, largest %r" % (len(P["d"]), zero, P["d"][P["d"] > 0].min(), P["d"].max()))
    assert zero == 0 and len(P["d"]) == shapes.BAND_N * (shapes.BAND_N - 1) // 2
    found = shapes.band_pairs()
    print("band pairs", found)
    cones = g3.Cones(sc["cones"])
    st, _ = shapes.so3_milestones(sc, shapes.BAND_N)
    for target, (j, i, d) in found.items():
        assert d == g3.distance(list(st[j]), list(st[i])) and g3.check_motion(cones, sc["fraction"], list(st[j]), list(st[i]))
        ad = abs(g3.dot(list(st[j]), list(st[i])))
        for r in shapes.band_radii(d):
            lo, hi = shapes.so3_radius_bands(r)
            assert lo <= ad <= hi                                       # decided by the exact distance, not by a band
            assert (i in shapes.so3_roadmap(sc, radius=r)["edges"][j]) == (d < r)
    assert 4.5e-5 < found["smallest"][2] < 0.04                          # beyond the 1 - 1e-9 cut, on the LERP side of 0.9995
    assert abs(found[0.0316][2] - 0.0316) < 2e-3 and abs(found[0.3][2] - 0.3) < 1e-3 and abs(found[1.0][2] - 1.0) < 1e-3
    assert g3.PIO2_HI - 1e-4 < found["largest"][2] <= g3.PIO2_HI
    for r in shapes.BAND_CUTOFF_RADII:                                   # nothing lies within them: no pair is closer than 4.47e-5
        assert shapes.so3_roadmap(sc, radius=r)["candidates"] == zero == 0
