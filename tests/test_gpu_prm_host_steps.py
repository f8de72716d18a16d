"""GPU: what the PRM host loop alone decides (oxhip_prm_api.hip), against tests/golden/prm_host_counters.json, the counters the
library of the commit named there reported for the same configs: milestones, edge entries, samples drawn, candidate pairs,
replayed sample batches, k-nearest rows searched exactly; the rounds and statuses of a chunked batch (one counter corrected since:
the file's "_corrected" entry, held to the oracle by tests/test_prm_limits_model.py).  Also the phase_ms slots
and the handle-level refusals, whose texts are the literals of that commit's source."""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import pytest

from prm_helpers import csr_checksum, states_checksum

pytestmark = pytest.mark.gpu

from oxmpl_amd import capi  # noqa: E402
from test_gpu_prm import make_gpu_prm  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_prm_host_counters as gen  # noqa: E402

with open(os.path.join(HERE, "golden", "prm_host_counters.json")) as _f:
    GOLDEN = json.load(_f)
CONFIGS = dict(gen.CONFIGS)


def test_the_file_names_its_commit_and_the_generators_configs():
    assert len(GOLDEN["_library_commit"]) == 40 and list(GOLDEN["configs"]) == [n for n, _ in gen.CONFIGS]
    g = GOLDEN["configs"]
    assert g["r2_radius"] == g["r2_radius_timeout"]                      # 600 < 4096: one round with or without the clock
    assert g["r3_knn_two_rounds"]["n_milestones"] == g["so3_radius_two_rounds"]["n_milestones"] == 5000   # 4096, then 5000
    assert g["r2_sample_cap"]["n_samples"] == 300 and g["r2_sample_cap"]["n_milestones"] < 1000
    assert g["r2_radius_zero"]["edge_entries"] == g["r2_radius_zero"]["n_candidates"] == 0
    assert GOLDEN["batch"]["rounds"] == 3 and len(GOLDEN["batch"]["statuses"]) == 8


@pytest.mark.parametrize("name", [n for n, _ in gen.CONFIGS])
def test_counters_and_phase_slots(name):
    g, counters, ms = gen.construct(CONFIGS[name])
    print(name, counters, ms)
    assert counters == GOLDEN["configs"][name]
    assert len(ms) == 6 and all(math.isfinite(v) and v >= 0.0 for v in ms)
    connects = CONFIGS[name]["radius"] > 0.0 or CONFIGS[name].get("knn_k", 0)
    assert ms[0] > 0.0                                                   # sampling ran
    if connects:
        assert ms[1] > 0.0 and ms[2] > 0.0 and ms[3] > 0.0               # pairs, edges, sort + CSR ran
    else:
        assert ms[1] == 0.0 and ms[2] == 0.0                             # no pair search, no edge check
    assert ms[4] == 0.0 and ms[5] == 0.0                                 # no query yet
    st, path = g.solve()
    t = g.last_timing()["phase_ms"]
    print(name, "solve", st, t)
    assert t[:4] == ms[:4] and math.isfinite(t[4]) and t[4] > 0.0 and math.isfinite(t[5]) and t[5] >= 0.0
    if name == "r2_radius":
        assert gen.batch(g) == GOLDEN["batch"]
        bt = g.batch_last_timing()["phase_ms"]
        print(name, "batch", bt)
        assert all(math.isfinite(v) and v >= 0.0 for v in bt) and bt[0] > 0.0 and bt[1] > 0.0
    g.close()


def _refused(L, status, want_status, want_text):
    assert status == want_status and L.oxhip_last_error_string().decode() == want_text


def test_handle_level_refusals_then_a_golden_roadmap(prm_golden):
    L = capi.lib()
    dp = C.POINTER(C.c_double)
    ln, buf = C.c_uint32(), (C.c_double * 64)()
    g = gen.make(CONFIGS["r2_radius"])
    _refused(L, L.oxhip_prm_construct_roadmap(g._h), capi.ERR_PLANNER_UNINITIALISED, "setup() was not called")
    _refused(L, L.oxhip_prm_solve(g._h, 0.0, None, 0, C.byref(ln)), capi.ERR_PLANNER_UNINITIALISED, "setup() was not called")
    cfg = CONFIGS["r2_radius"]
    g.setup(cfg["start"], cfg["goal"], cfg["goal_r"])
    _refused(L, L.oxhip_prm_solve(g._h, 0.0, None, 0, C.byref(ln)), capi.ERR_UNSAMPLED_STATE_SPACE, "construct_roadmap() left no milestones")
    s = gen.make(CONFIGS["so3_radius_two_rounds"])
    lo = (C.c_double * 4)(0.0, 0.0, 0.0, 0.0)
    _refused(L, L.oxhip_prm_set_boxes(s._h, C.cast(lo, dp), C.cast(lo, dp), 1), capi.ERR_BAD_ARG,
             "SO(3) PRM takes cones (oxhip_prm_set_spheres with 4-wide centres), not boxes")
    s.close()
    g.construct_roadmap()
    n, entries, _ = g.sizes()
    assert n == 600
    states = np.zeros((n, 2))
    _refused(L, L.oxhip_prm_get_roadmap(g._h, states.ctypes.data_as(dp), n - 1, None, None, 0), capi.ERR_CAPACITY, "roadmap buffers too small")
    nb = np.zeros(entries, dtype=np.uint32)
    _refused(L, L.oxhip_prm_get_roadmap(g._h, None, 0, None, nb.ctypes.data_as(C.POINTER(C.c_uint32)), entries - 1), capi.ERR_CAPACITY,
             "neighbour buffer too small")
    # query 5 of the generator's batch, which the recorded library solved: the path has at least 2 states
    g.set_problem(gen.BATCH["starts"][5], gen.BATCH["goals"][5], gen.BATCH["radii"][5])
    assert GOLDEN["batch"]["statuses"][5] == capi.OK
    assert L.oxhip_prm_solve(g._h, 0.0, None, 0, C.byref(ln)) == capi.OK and ln.value >= 2
    _refused(L, L.oxhip_prm_solve(g._h, 0.0, C.cast(buf, dp), ln.value - 1, C.byref(ln)), capi.ERR_CAPACITY, "path buffer too small")
    g.close()
    # after the refusals, in the same process: the golden scene, bit for bit
    P, R = prm_golden["wall"]["params"], prm_golden["wall"]["run"]
    q0 = R["queries"][0]
    w = make_gpu_prm(P)
    w.setup(q0["start"], q0["goal_c"], q0["goal_r"])
    w.construct_roadmap()
    assert w.sizes() == (R["n"], R["edge_entries"], R["n_samples"])
    ws, woff, wn = w.roadmap()
    assert "%016x" % states_checksum(ws) == R["states_checksum"] and "%016x" % csr_checksum(woff, wn) == R["csr_checksum"]
