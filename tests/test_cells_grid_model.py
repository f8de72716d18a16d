"""The grid model of tests/test_gpu_cells_limits.py against the source of rrt_cells.hip (no GPU): the cells_G table, the fill
and brute-list defaults, the limits the model uses, and the level sizes they give.  The GPU module places its cuts and proves
its crowding with the model, so a kernel change that moves a level must show up here first."""
import os
import re

import numpy as np

import test_gpu_cells_limits as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oxmpl_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_model_constants_match_the_kernel_source():
    src = _source("rrt_cells.hip")
    table = re.search(r"const uint32_t t\[15\] = \{([^}]*)\};", src)
    assert table is not None
    assert tuple(int(v.strip().rstrip("u")) for v in table.group(1).split(",")) == model.G_TABLE
    assert int(re.search(r"#define OXHIP_CELLS_FILL_X2 (\d+)ull", src).group(1)) == model.FILL_X2
    assert int(re.search(r"#define OXHIP_CELLS_BRUTE (\d+)\n", src).group(1)) == model.BRUTE
    assert int(re.search(r"constexpr uint32_t kFlatCap = (\d+);", src).group(1)) == model.FLAT_CAP
    assert int(re.search(r"constexpr uint32_t kMaxSplit = (\d+);", src).group(1)) == model.MAX_SPLIT
    assert int(re.search(r"constexpr int kMaxShell = (\d+);", src).group(1)) == model.MAX_SHELL
    lim = re.search(r"const uint32_t lim = dim == 2 \? (\d+)u : (\d+)u;", src)
    assert (int(lim.group(1)), int(lim.group(2))) == (model.LEVEL_LIM[2], model.LEVEL_LIM[3])
    assert int(re.search(r"\(dim == 2 \|\| dim == 3\) && cap <= (\d+)u;", src).group(1)) == model.CAP_LIMIT
    # the capacity: max_nodes rounded up to 1024, and the kernel's refusal names the largest max_nodes it takes
    api = _source("oxhip_api.hip")
    assert "const uint32_t cap = ((cfg->max_nodes + 1023u) / 1024u) * 1024u;" in api
    assert "cell-grid kernel: R^2 / R^3 trees of at most 64,512 nodes" in api
    assert model.capacity(64512) <= model.CAP_LIMIT < model.capacity(64513)


def test_model_level_sizes():
    # regrid sizes (cap + 1 per level) and the finest level's cap for the largest capacity
    assert model.regrid_sizes(2, 64512) == [513, 897, 1852, 3585, 7088, 14337, 28984]
    assert model.cells_level_cap(model.cells_level_max(2, 64512), 2) == 57344
    assert model.regrid_sizes(3, 64512) == [513, 757, 1793, 4659, 14337, 42585]
    assert model.cells_level_max(3, 64512) == model.LEVEL_LIM[3]
    # a level serves trees up to its cap; the next node moves the tree on
    for dim in (2, 3):
        lmax = model.cells_level_max(dim, 64512)
        assert model.cells_level(model.BRUTE, dim, lmax) == 0 and model.cells_level(model.BRUTE + 1, dim, lmax) > 0
        for t in model.regrid_sizes(dim, 64512)[1:]:
            assert model.cells_level(t, dim, lmax) > model.cells_level(t - 1, dim, lmax)
    # the shape variants change the sizes, never the results: the counter bound takes the fewest level changes
    assert model.regrid_sizes(2, 15000, fill_x2=64) == [513, 1153, 2049, 3873, 8193]
    assert model.regrid_sizes(3, 15000, brute=64)[:3] == [65, 95, 225]
    assert model.regrids_below(2, 15000) == 5 and model.regrids_below(3, 15000) == 4


def test_model_box_and_cells():
    # the box is bounds u goal centre u tree; the longest side has G cells, a thin axis one; the upper face clamps inward
    states = np.array([[0.0, 0.0, 0.0], [10.0, 10.0, 1e-8], [5.0, 5.0, 5e-9]])
    lo, inv_h, gk = model.grid_of(states, 3, [(0.0, 10.0), (0.0, 10.0), (0.0, 1e-8)], [10.0, 10.0, 1e-8], 5000)
    assert list(gk) == [1, 1, 1]   # (three nodes: the brute list's level 0, one cell)
    many = np.vstack([states, np.random.default_rng(0).random((3000, 3)) * [10.0, 10.0, 1e-8]])
    lo, inv_h, gk = model.grid_of(many, many.shape[0], [(0.0, 10.0), (0.0, 10.0), (0.0, 1e-8)], [10.0, 10.0, 1e-8], 5000)
    assert list(gk) == [11, 11, 1]
    assert model.cell_of([10.0, 10.0, 1e-8], lo, inv_h, gk).tolist() == [10, 10, 0]
    assert model.cell_of([0.0, 0.0, 0.0], lo, inv_h, gk).tolist() == [0, 0, 0]
    # a goal centre 10^4 away puts a tree in [0, 10]^2 into one cell
    pts = np.random.default_rng(1).random((5000, 2)) * 10.0
    assert model.fullest_cell(pts, 5000, [(0.0, 10.0)] * 2, [1e4, 1e4], 15000) == 5000
    # duplicates (-0.0 == +0.0) are filed once
    dup = np.array([[0.0, 1.0], [-0.0, 1.0], [0.0, 1.0], [2.0, 3.0], [2.0, 3.0]])
    assert model.filed_nodes(dup).shape[0] == 2
