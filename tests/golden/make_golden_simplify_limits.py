"""Writes tests/golden/simplify_limits.json: the shortcut of DESIGN.md section 18 over the planted paths of
tests/simplify_limits_shapes.py, by the CPU oracle alone -- never the device.

R^n: oracle_py.OracleRRT.check_motion, oracle_py.distance and simplify_helpers.shortcut_dp.  so3_arc: make_golden_so3's check_motion
and distance.  Per scene, problem and span: L, the simplified path's indices, raw and simplified cost as hex floats, the number of
motion checks and the number of valid pairs among those checked ("valid").  Scenes marked `matrix` also record every verdict at full
span: "matrix" = the pairs (i, j), j - i >= 2, ROW-MAJOR (i ascending, then j ascending), one bit per pair, packed most significant
bit first (numpy.packbits) and written as hex.

    python tests/golden/make_golden_simplify_limits.py
"""
import functools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import make_golden_so3 as so3  # noqa: E402
import simplify_helpers as sh  # noqa: E402
import simplify_limits_shapes as shapes  # noqa: E402

OUT = os.path.join(HERE, "simplify_limits.json")


def rn_oracle(scene, problem, without=None):
    """the scene's checker as an OracleRRT; `without`: an obstacle index (spheres first, then boxes) left out"""
    from oracle import oracle_py as orc
    o = orc.OracleRRT(scene["dim"], scene["bounds"], 0.5, 0.05, scene["lvs_fraction"], scene["max_nodes"], True, 0, 0)
    c, r = scene["spheres"]
    ns = len(r)
    keep = [k for k in range(ns) if k != without]
    if keep:
        o.set_spheres(c[keep], r[keep])
    if scene["boxes"] is not None:
        lo, hi = scene["boxes"]
        keepb = [k for k in range(len(lo)) if ns + k != without]
        if keepb:
            o.set_boxes(lo[keepb], hi[keepb])
    o.setup(problem["states"][0], problem["goal"][0], problem["goal"][1])
    return o


@functools.lru_cache(maxsize=None)
def analysis(name, p):
    """(L, valid {(i, j): bool}, dist(i, j)) of problem p: every pair the scene's widest span checks, computed once"""
    from oracle import oracle_py as orc
    scene = shapes.scenes()[name]()
    problem = scene["problems"][p]
    L = shapes.length(problem)
    if L == 0:
        return 0, {}, None
    path = problem["path"]
    S = max(sh.span_of(L, s) for s in shapes.spans_of(name, scene, p))
    if scene["so3"]:
        rows = [[float(v) for v in q] for q in path]
        cones = so3.Cones([(list(c), float(r)) for c, r in zip(*scene["spheres"])])
        check = lambda i, j: so3.check_motion(cones, scene["lvs_fraction"], rows[i], rows[j])  # noqa: E731
        raw_dist = lambda i, j: so3.distance(rows[i], rows[j])  # noqa: E731
    else:
        o = rn_oracle(scene, problem)
        check = lambda i, j: o.check_motion(path[i], path[j])  # noqa: E731
        raw_dist = lambda i, j: orc.distance(path[i], path[j])  # noqa: E731
    valid = {(i, j): bool(check(i, j)) for i in range(L) for j in range(i + 2, min(L, i + S + 1))}
    dist = functools.lru_cache(maxsize=None)(raw_dist)
    return L, valid, dist


def result(name, p, span):
    L, valid, dist = analysis(name, p)
    return sh.shortcut_dp(L, lambda i, j: valid[(i, j)], dist, span)


def matrix_pairs(L):
    return [(i, j) for i in range(L) for j in range(i + 2, L)]


def pack(bools):
    return np.packbits(np.asarray(bools, dtype=np.uint8)).tobytes().hex()


def unpack(hexed, n):
    return np.unpackbits(np.frombuffer(bytes.fromhex(hexed), dtype=np.uint8))[:n].astype(bool)


def record(name, scene, p):
    L, valid, _ = analysis(name, p)
    rec = dict(L=L, goal_node=scene["problems"][p]["goal_node"], spans={})
    for span in shapes.spans_of(name, scene, p):
        idx, raw, cost, checks = result(name, p, span)
        S = sh.span_of(L, span) if L else 0
        rec["spans"][str(span)] = dict(idx=idx, raw=mg.hexf(raw), cost=mg.hexf(cost), checks=checks,
                                       valid=sum(v for (i, j), v in valid.items() if j - i <= S))
    if scene["matrix"]:
        rec["matrix"] = pack([valid[ij] for ij in matrix_pairs(L)])
    return rec


def build():
    out = {"_generator": "tests/golden/make_golden_simplify_limits.py",
           "_parity": "UNPINNED: the reference has no path simplifier; the semantics are include/oxmpl_hip.h's",
           "_matrix": "pairs (i, j), j - i >= 2, row-major, numpy.packbits (most significant bit first), hex"}
    for name, make in shapes.scenes().items():
        scene = make()
        out[name] = [record(name, scene, p) for p in range(len(scene["problems"]))]
    return out


def dumps(out):
    return json.dumps(out, separators=(",", ":"), sort_keys=True) + "\n"


def main():
    out = build()
    with open(OUT, "w") as f:
        f.write(dumps(out))
    print("wrote", OUT, {k: [(r["L"], len(r["spans"])) for r in v] for k, v in out.items() if isinstance(v, list)})


if __name__ == "__main__":
    main()
