"""Writes tests/golden/prm_host_counters.json: the counters that the PRM host loop alone decides (oxhip_prm_api.hip: the sizes
of the sampling rounds, the doubling rounds under a wall clock, the k-nearest shortfall rows, the rounds of a chunked batch),
for a handful of small configs, as the library that writes the file reports them.

The file is a record of the library BEFORE a change to the host code: build the commit to be pinned, run this against it on a
GPU and name the commit, then replay the file against the changed library (tests/test_gpu_prm_host_steps.py).

    OXMPL_HIP_LIB=<that commit's liboxmpl_hip.so> python tests/golden/make_golden_prm_host_counters.py <commit> [out.json]
"""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oxmpl_amd import capi  # noqa: E402

R2 = dict(dim=2, bounds=[0.0, 10.0, 0.0, 10.0], radius=0.5, max_milestones=600, seed=3, stream=0,
          boxes=([[4.5, 2.0]], [[5.5, 8.0]]), start=[1.0, 5.0], goal=[9.0, 5.0], goal_r=0.5)
# (name, config): every one a few seconds or less; a finite timeout of 60 s is never reached, it only switches the doubling rounds on
CONFIGS = [
    ("r2_radius", R2),
    ("r2_radius_timeout", dict(R2, timeout=60.0)),
    ("r3_knn_two_rounds", dict(dim=3, bounds=[0.0, 10.0] * 3, radius=1.0, knn_k=4, max_milestones=5000, timeout=60.0, seed=42, stream=1,
                               spheres=([[5.0, 5.0, 5.0], [2.0, 7.0, 3.0]], [2.0, 1.5]), start=[0.5] * 3, goal=[9.5] * 3, goal_r=1.0)),
    ("so3_radius_two_rounds", dict(dim=4, space=capi.SPACE_SO3, bounds=[0.0, 0.0, 0.0, 1.0, math.pi], radius=0.3, max_milestones=5000,
                                   timeout=60.0, seed=5, stream=2, spheres=([[1.0, 0.0, 0.0, 0.0]], [0.6]),
                                   start=[0.0, 0.0, 0.0, 1.0], goal=[0.0, 1.0, 0.0, 0.0], goal_r=0.3)),
    ("r2_sample_cap", dict(R2, max_milestones=1000, max_samples=300)),
    ("r2_radius_zero", dict(R2, radius=0.0)),
    ("r2_radius_negative", dict(R2, radius=-1.0)),
]
# 8 queries on the r2_radius roadmap, answered 3 to a round: two starts lie in the box
BATCH = dict(starts=[[1.0, 5.0], [5.0, 5.0], [9.0, 9.0], [0.5, 0.5], [4.6, 7.9], [2.0, 8.0], [8.0, 1.0], [3.0, 3.0]],
             goals=[[9.0, 5.0], [9.0, 5.0], [1.0, 1.0], [9.5, 9.5], [1.0, 1.0], [8.0, 2.0], [2.0, 9.0], [20.0, 20.0]],
             radii=[0.5] * 8, chunk_queries=3)


def make(cfg):
    g = capi.PRMRoadmap(cfg["dim"], cfg["bounds"], cfg["radius"], cfg["max_milestones"], timeout=cfg.get("timeout", 0.0),
                        max_samples=cfg.get("max_samples", 0), seed=cfg["seed"], stream=cfg["stream"], knn_k=cfg.get("knn_k", 0),
                        space=cfg.get("space", capi.SPACE_REAL_VECTOR))
    if "spheres" in cfg:
        g.set_spheres(*cfg["spheres"])
    if "boxes" in cfg:
        g.set_boxes(*cfg["boxes"])
    return g


def construct(cfg):
    """(the roadmap's handle, its counters, phase_ms of the construction)"""
    g = make(cfg)
    g.setup(cfg["start"], cfg["goal"], cfg["goal_r"])
    g.construct_roadmap()
    n, entries, samples = g.sizes()
    t = g.last_timing()
    counters = dict(n_milestones=n, edge_entries=entries, n_samples=samples, n_candidates=t["candidates"],
                    redraw_batches=t["redraw_batches"], knn_exact_rows=g.knn_exact_rows())
    return g, counters, t["phase_ms"]


def batch(g):
    st = g.solve_batch(BATCH["starts"], BATCH["goals"], BATCH["radii"], chunk_queries=BATCH["chunk_queries"])
    return dict(rounds=g.batch_last_timing()["rounds"], statuses=[int(s) for s in st])


def main():
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "prm_host_counters.json")
    assert capi.device_count() > 0, "write this file on a machine with a GPU"
    doc = {"_generator": "tests/golden/make_golden_prm_host_counters.py", "_library_commit": commit, "configs": {}}
    for name, cfg in CONFIGS:
        g, counters, _ = construct(cfg)
        doc["configs"][name] = counters
        if name == "r2_radius":
            doc["batch"] = batch(g)
        g.close()
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
