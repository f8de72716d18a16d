#!/usr/bin/env python3
"""Generates tests/golden/prm_revalidate.json: roadmaps re-checked after obstacles were added (oxhip_prm_revalidate, DESIGN.md
section 20), by a pure-Python restatement on top of the pieces of make_golden_prm.py / make_golden_prm_knn.py /
make_golden_prm_so3.py (prm_construct, is_valid, check_motion).

The semantics are the build's own (the reference has no such call): valid[i] = is_valid(milestone i) in the NEW scene; an
undirected edge {i < j} is kept iff valid[i], valid[j] and check_motion(from = milestone j, to = milestone i), the direction in
which construction checked it (prm.rs:134); an invalid milestone keeps its index and loses its entries; rows stay ascending.

Per scene: the roadmap's checksums before (states, CSR), the added obstacles, the valid mask (as the invalid indices), the
filtered CSR's checksum and size -- and, for the small scene r2_small, the filtered CSR in full.  The other roadmaps (up to
14,848 entries) are not stored: the tests rebuild them.  Each
scene is asserted not to be vacuous: a milestone becomes invalid, an edge between two still-valid milestones is removed, an
edge survives.

"direction": check_motion tests the states from + (to - from) i / n, i = 1 .. n, so a -> b and b -> a test points that differ in
their last bits.  The search draws random pairs in [0,10]^2 and a sphere that GRAZES the motion a -> b -- its radius is the
smallest centre distance among the states that a -> b tests, which (validity being strict) makes a -> b invalid by one
comparison -- and keeps the first pair, of at most 10^6, whose opposite motion b -> a is valid while both ends are.

Run:  python tests/golden/make_golden_prm_revalidate.py      (about a minute, most of it the SO(3) roadmap)
"""
import json
import os
import random
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import make_golden_prm as mp  # noqa: E402
import make_golden_prm_knn as mk  # noqa: E402
import make_golden_prm_so3 as mp3  # noqa: E402
import make_golden_so3 as g3  # noqa: E402

hx = lambda row: [mg.hexf(float(v)) for v in row]  # noqa: E731


def revalidate(states, edges, is_valid, check_motion):
    """(valid mask, filtered edge lists): the plain filter"""
    n = len(edges)
    valid = [bool(is_valid(states[i])) for i in range(n)]
    keep = [[] for _ in range(n)]
    for j in range(n):
        for i in edges[j]:
            if i < j and valid[i] and valid[j] and check_motion(states[j], states[i]):   # from the higher index to the lower
                keep[j].append(i)
                keep[i].append(j)
    return valid, [sorted(e) for e in keep]


def not_vacuous(name, edges, valid, kept):
    removed_between_valid = sum(1 for j in range(len(edges)) for i in edges[j] if i < j and valid[i] and valid[j] and i not in kept[j])
    assert not all(valid), name + ": no milestone became invalid"
    assert removed_between_valid > 0, name + ": no edge between two valid milestones was removed"
    assert sum(len(e) for e in kept) > 0, name + ": no edge survived"
    return removed_between_valid


def record(name, params, states, edges, added, valid, kept, full=False):
    cut = not_vacuous(name, edges, valid, kept)
    print(name, "n", len(edges), "entries", sum(len(e) for e in edges), "->", sum(len(e) for e in kept), "invalid", valid.count(False),
          "edges cut between valid milestones", cut)
    # compact on purpose: the roadmap itself is not stored -- the tests rebuild it (C oracle, device, this generator) and pin it by
    # its checksums; the valid mask is the list of invalid indices, the filtered CSR its checksum and size
    return dict(params=params, n=len(edges), entries_before=sum(len(e) for e in edges),
                csr_checksum_before="%016x" % mp.csr_checksum(edges), states_checksum="%016x" % mp.states_checksum(states),
                added=added, invalid=[i for i, v in enumerate(valid) if not v], cut_between_valid=cut,
                csr_checksum_after="%016x" % mp.csr_checksum(kept), entries_after=sum(len(e) for e in kept),
                removed_entries=sum(len(e) for e in edges) - sum(len(e) for e in kept), n_invalid=valid.count(False),
                **(dict(edges_after=kept) if full else {}))   # the filtered CSR in full where it is small


def rn_scene(name, P, added_spheres, added_boxes=(), full=False):
    """an R^n scene: construct in P's obstacles, re-check with the added ones on top"""
    spheres0 = [(unhex_row(c), unhex(r)) for c, r in P["spheres"]]
    f0 = mg.Field(P["dim"], spheres0, P["boxes"])
    if P.get("knn_k"):
        rm = mk.prm_construct_knn(P["dim"], P["bounds"], P["knn_k"], P["fraction"], f0, P["seed"], P["stream"], P["max_milestones"], 10 ** 9)
    else:
        rm = mp.prm_construct(P["dim"], P["bounds"], P["radius"], P["fraction"], f0, P["seed"], P["stream"], P["max_milestones"], 10 ** 9)
    assert len(rm["edges"]) == P["max_milestones"]
    states = [[float(v) for v in row] for row in rm["states"]]
    f1 = mg.Field(P["dim"], spheres0 + list(added_spheres), list(P["boxes"]) + list(added_boxes))
    valid, kept = revalidate(states, rm["edges"], f1.is_valid, lambda a, b: mg.check_motion(f1, P["bounds"], P["fraction"], a, b))
    added = dict(spheres=[[hx(c), mg.hexf(r)] for c, r in added_spheres], boxes=[[list(lo), list(hi)] for lo, hi in added_boxes])
    return record(name, P, states, rm["edges"], added, valid, kept, full)


def unhex(h):
    """the inverse of make_golden.hexf (the 16 hex digits of the binary64 pattern)"""
    return struct.unpack("<d", struct.pack("<Q", int(h, 16)))[0]


def unhex_row(row):
    return [unhex(v) for v in row]


def so3_scene(name, sc, added_cones):
    cones0 = g3.Cones(sc["cones"])
    rm = mp3.prm_construct(sc["bounds"], sc["radius"], sc["fraction"], cones0, sc["seed"], sc["stream"], sc["max_milestones"], sc["max_samples"])
    assert len(rm["states"]) == sc["max_milestones"]
    cones1 = g3.Cones(list(sc["cones"]) + list(added_cones))
    valid, kept = revalidate(rm["states"], rm["edges"], cones1.is_valid, lambda a, b: g3.check_motion(cones1, sc["fraction"], a, b))
    added = dict(cones=[[hx(c), mg.hexf(r)] for c, r in added_cones])
    return record(name, mp3.scene_params(dict(sc, queries=[])), rm["states"], rm["edges"], added, valid, kept)


def direction_scene(max_tries=10 ** 6):
    """a pair (a, b), both valid, and a sphere with check_motion(a -> b) invalid and check_motion(b -> a) valid"""
    bounds, fraction = [(0.0, 10.0), (0.0, 10.0)], 0.05
    rnd = random.Random(20261019)
    lvsl = mg.maximum_extent(bounds) * fraction
    for tries in range(1, max_tries + 1):
        a = [rnd.uniform(1.0, 9.0), rnd.uniform(1.0, 9.0)]
        b = [a[0] + rnd.uniform(-0.7, 0.7), a[1] + rnd.uniform(-0.7, 0.7)]
        t0 = rnd.uniform(0.3, 0.7)
        c = [a[0] + (b[0] - a[0]) * t0 + rnd.uniform(-0.2, 0.2), a[1] + (b[1] - a[1]) * t0 + rnd.uniform(-0.2, 0.2)]
        n = mg.num_steps(mg.distance(a, b), lvsl)
        if n < 4:
            continue
        r = min(mg.distance(c, mg.interpolate(a, b, float(i) / float(n))) for i in range(1, n + 1))   # grazes a -> b
        field = mg.Field(2, [(c, r)])
        if not (field.is_valid(a) and field.is_valid(b)):
            continue
        ab, ba = mg.check_motion(field, bounds, fraction, a, b), mg.check_motion(field, bounds, fraction, b, a)
        assert not ab
        if ba:
            print("direction: found after", tries, "pairs")
            return dict(found=True, tries=tries, bounds=bounds, fraction=fraction, a=hx(a), b=hx(b), sphere=[hx(c), mg.hexf(r)],
                        a_to_b=bool(ab), b_to_a=bool(ba))
    print("direction: none found in", max_tries, "pairs")
    return dict(found=False, tries=max_tries, bounds=bounds, fraction=fraction)


def _so3():
    # SO(3), 512 milestones: the reference's fixture scene (one cone about the identity); two cones are added
    fx = mp3.fixture_scene()
    sc = dict(fx, seed=25, stream=1, max_milestones=512)
    return so3_scene("so3", sc, [(g3.normalise([0.6, 0.1, -0.3, 0.7]), 0.35), (g3.normalise([-0.2, 0.7, 0.5, 0.4]), 0.25)])


def scenes(only=None):
    out = {}
    if only == "so3":
        return dict(so3=json.loads(json.dumps(_so3())))
    # R^2, radius rule, 600 milestones: the reference's wall scene with a wider radius; three discs are added
    p2 = dict(dim=2, bounds=[(0.0, 10.0), (0.0, 10.0)], radius=0.8, fraction=0.05, spheres=[], boxes=[([4.75, 2.0], [5.25, 8.0])],
              seed=21, stream=0, max_milestones=600, max_samples=10 ** 9)
    out["r2_radius"] = rn_scene("r2_radius", p2, [([2.5, 6.5], 0.9), ([7.25, 3.0], 0.6), ([8.0, 8.5], 0.35)], [([1.0, 1.0], [1.9, 1.3])])
    # the same scene small (120 milestones, wider radius): its filtered CSR is stored in full, so that a checksum that differs
    # elsewhere can be diagnosed from one that can be read
    ps = dict(p2, radius=1.3, seed=27, max_milestones=120)
    out["r2_small"] = rn_scene("r2_small", ps, [([2.5, 6.5], 0.9), ([7.25, 3.0], 0.6), ([8.0, 8.5], 0.35)], [([1.0, 1.0], [1.9, 1.3])], full=True)
    # R^6, k-nearest (k = 8), 400 milestones: the 16-hypersphere field of prm_knn_golden's r6_k8; two hyperspheres are added
    s6, g6 = [3.0] * 6, [7.0] * 6
    sph6 = mg.sphere_field(0x5EED0006, 16, 6, 1.0, 9.0, 3.0, 4.5, [s6, g6])
    p6 = dict(dim=6, bounds=[(0.0, 10.0)] * 6, radius=4.0, knn_k=8, fraction=0.05, boxes=[], seed=23, stream=2, max_milestones=400,
              max_samples=10 ** 9, spheres=[[hx(c), mg.hexf(r)] for c, r in sph6])
    out["r6_knn"] = rn_scene("r6_knn", p6, [([5.0, 5.0, 4.0, 6.0, 5.0, 5.0], 3.2), ([2.0, 8.0, 2.0, 8.0, 2.0, 8.0], 3.6)])
    out["so3"] = _so3()
    out["direction"] = direction_scene()
    return out


def main():
    out = {"_generator": "tests/golden/make_golden_prm_revalidate.py"}
    out.update(scenes())
    path = os.path.join(HERE, "prm_revalidate.json")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(out[k], sort_keys=True)) for k in sorted(out)) + "\n}\n")   # a line per scene
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
