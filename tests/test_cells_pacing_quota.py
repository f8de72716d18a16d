"""CPU: the progress units of a frozen cell-grid launch's pacing (rrt_cells.hip, cells_part_quota), through the
host-callable functions the library exports.  A launch of `rounds` rounds cut into `split` parts: a round a part runs counts
OXHIP_CELLS_SKIP_COST_INV = 16 units, a round it skips on the way to its own start counts 1 (launches of up to kSelfSkipMax = 4
parts; with more parts the prepare pass finds the starts and nothing is skipped).  Every wave of an XCD compares its own fraction
done with the fraction the XCD's board shows of the XCD's quota, which it knows from the launch geometry alone -- so the parts'
quotas must add up to exactly what the host hands the kernel, or the board never shows 100 %."""
import os
import re

import pytest

from oxmpl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS = range(0, 201)
SPLITS = range(1, 65)


@pytest.fixture(scope="module")
def L():
    capi.build_library()
    return capi.lib()


@pytest.fixture(scope="module")
def knobs():
    src = open(os.path.join(ROOT, "oxmpl_amd", "csrc", "rrt_cells.hip")).read()
    unit = int(re.search(r"#define OXHIP_CELLS_SKIP_COST_INV (\d+)\n", src).group(1))
    self_skip = int(re.search(r"constexpr uint32_t kSelfSkipMax = (\d+);", src).group(1))
    max_split = int(re.search(r"constexpr uint32_t kMaxSplit = (\d+);", src).group(1))
    assert (unit, self_skip, max_split) == (16, 4, 64)
    assert re.search(r"#define OXHIP_CELLS_PACE_BAND OXHIP_CELLS_SKIP_COST_INV ", src)   # the dead band: one round
    return unit, self_skip


def test_parts_tile_the_rounds(L):
    for split in SPLITS:
        for rounds in ROUNDS:
            b = [L.oxhip_cells_part_begin(rounds, part, split) for part in range(split + 2)]
            assert b[0] == 0 and b[split] == rounds and b[split + 1] == rounds
            assert all(b[i] <= b[i + 1] for i in range(split + 1))


def test_quotas_are_what_the_parts_run_and_skip(L, knobs):
    unit, self_skip = knobs
    for split in SPLITS:
        for rounds in ROUNDS:
            begin = [L.oxhip_cells_part_begin(rounds, part, split) for part in range(split + 1)]
            quota = [L.oxhip_cells_part_quota(rounds, part, split) for part in range(split)]
            skips = 1 < split <= self_skip
            for part in range(split):
                # (an unsigned 64-bit value that had gone below zero would be huge)
                assert 0 <= quota[part] <= (unit + 1) * rounds
                assert quota[part] == unit * (begin[part + 1] - begin[part]) + (begin[part] if skips else 0)
            total = L.oxhip_cells_problem_quota(rounds, split)
            assert sum(quota) == total
            if split <= self_skip:
                assert total == unit * rounds + (sum(begin[:split]) if skips else 0)
            else:
                assert total == unit * rounds
            assert L.oxhip_cells_part_quota(rounds, split, split) == 0          # no such part
            assert L.oxhip_cells_part_quota(rounds, split + 7, split) == 0


def test_arguments_out_of_range_give_nothing(L):
    for split in (0, 65, 2 ** 32 - 1):
        assert L.oxhip_cells_part_quota(100, 0, split) == 0
        assert L.oxhip_cells_problem_quota(100, split) == 0
        assert L.oxhip_cells_part_begin(100, 0, split) == 100


def test_flag_and_stamp_word_are_mirrored():
    header = open(os.path.join(ROOT, "include", "oxmpl_hip.h")).read()
    assert int(re.search(r"OXHIP_DEBUG_CELLS_NO_PACING\s*=\s*(\d+)", header).group(1)) == capi.DEBUG_CELLS_NO_PACING == 2048
    assert int(re.search(r"#define OXHIP_STAMP_CELLS_BOARD\s+(\d+)", header).group(1)) == capi.STAMP_CELLS_BOARD == 3
