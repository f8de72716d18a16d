"""-m gpu: a bounded leg of the randomised parity sweep (tools/fuzz_parity.py) inside the suite the driver runs, with fixed
seeds: random spaces (dim 1-8, offsets to 1e6; RRTConnect and SE(2) also scaled to 1e-12 and beyond binary32), obstacle
fields, planner parameters, batch sizes, resume splits, frozen legs; every planner and kernel kind against its CPU oracle, bit
for bit.  The lane-per-query kernel's rarely taken paths (whole-tree
path, memoized answers, one-lane rounds, two-lane passes) are forced in about half of its cases through
oxhip_rrt_config.debug_flags.  VERDICT round 2: a wrong accept in that kernel's whole-tree path was found by the sweep only."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.mark.parametrize("seed,seconds,only", [(3101, 45.0, None), (3102, 40.0, "rrt"), (3103, 25.0, "rrt_star"), (3104, 25.0, "se2_connect"),
                                                  (3105, 25.0, "se2_connect"), (3106, 25.0, "rrt_connect")])
def test_fuzz_leg_has_no_mismatch(seed, seconds, only):
    import fuzz_parity
    counts, failures = fuzz_parity.sweep(seconds, seed, only, verbose=False)
    print("fuzz seed %d: %s" % (seed, counts))
    assert sum(counts.values()) >= 20, counts     # the leg really ran
    assert failures == []
