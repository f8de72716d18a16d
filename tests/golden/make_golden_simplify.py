"""Writes tests/golden/simplify_golden.json: the shortcut of DESIGN.md section 18 over the CPU oracle's own paths.

R^n: oracle_py.OracleRRT / OracleRRTStar (path(), check_motion(), oracle_py.distance) on config 1, config 2 and the wall at
seed 42, problems 0 .. 7, and RRT* on config 1 for 2 problems.  SO(3): make_golden_so3's rrt_solve / check_motion / distance on
the fixture scene, 4 problems.  Per problem and span: the raw length, the simplified path's indices, both costs as hex floats
and the number of motion checks.  RRTConnect has no oracle check_motion and so no record here.

    python tests/golden/make_golden_simplify.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import make_golden_so3 as so3  # noqa: E402
import simplify_helpers as sh  # noqa: E402

SPANS = (0, 3)
RN_PROBLEMS = 8
STAR_PROBLEMS = 2
STAR_RADIUS = 1.0
SO3_PROBLEMS = 4


def _record(pid, L, results):
    return dict(pid=pid, L=L, spans={str(s): dict(idx=idx, raw=mg.hexf(raw), cost=mg.hexf(cost), checks=checks)
                                     for s, (idx, raw, cost, checks) in results.items()})


def rn_records(sc, pids, star_radius=None):
    out = []
    for pid in pids:
        if star_radius is None:
            o = sh.oracle_rrt(sc, pid)
            o.solve(sh.BUDGET)
        else:
            o = sh.oracle_rrt(sc, pid, star_radius, max_nodes=4000, stop_at_goal=False)
            o.solve(sh.STAR_ITERATIONS)
        path = o.path()
        assert o.goal_node >= 0 and len(path) >= 2, (pid, o.goal_node)
        out.append(_record(pid, len(path), {s: sh.oracle_shortcut(o, path, s) for s in SPANS}))
    return out


def so3_records(pids):
    sc = so3.fixture_scene()
    cones = so3.Cones(sc["cones"])
    out = []
    for pid in pids:
        path = so3.run_scene(sc, sh.SEED, pid)["path"]
        assert len(path) >= 2, pid
        res = {s: sh.shortcut_dp(len(path), lambda i, j: so3.check_motion(cones, sc["fraction"], path[i], path[j]),
                                 lambda i, j: so3.distance(path[i], path[j]), s) for s in SPANS}
        out.append(_record(pid, len(path), res))
    return out


def build():
    out = {"_generator": "tests/golden/make_golden_simplify.py", "seed": sh.SEED,
           "_parity": "UNPINNED: the reference has no path simplifier; the semantics are include/oxmpl_hip.h's"}
    for name, sc in sh.rn_scenes().items():
        out[name] = rn_records(sc, range(RN_PROBLEMS))
    out["config1_star"] = rn_records(sh.rn_scenes()["config1"], range(STAR_PROBLEMS), STAR_RADIUS)
    out["so3_fixture"] = so3_records(range(SO3_PROBLEMS))
    return out


def main():
    out = build()
    path = os.path.join(HERE, "simplify_golden.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote", path, {k: [(r["L"], len(r["spans"]["0"]["idx"])) for r in v] for k, v in out.items() if isinstance(v, list)})


if __name__ == "__main__":
    main()
