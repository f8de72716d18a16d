"""The band rule of rrt_cells.hip's frozen launches (cells_band_resolve) as a numpy model on the kernel's own
quantisation, against the reference's loop (rrt.rs:187-196: sqrt, strict '<', ascending index).  No GPU.

An ambiguous query is settled among the BAND: the nodes of the 3^D block of cells around the query whose binary32 screen
value is within thr2 = (sqrt(s1) (1 + 2^-20) + 2A)^2 of the query, s1 the smallest screen value, A the bound on a screen
distance's error.  The rule claims: if the band bound B is below the distance lb to the block's nearest open face, the band
holds the reference's nearest node, and the lexicographic minimum of (binary64 distance, index) over the band IS the
reference's answer.  The model below files nodes as cell_place does (16 bits per cell, decoded at the bin centre), screens
them as block_eval does (binary32, fused multiply-adds), computes A as the kernel does, and checks both claims over random
point sets and adversarial ones: exact ties, near-ties at every spacing from 0 to 4A, pairs straddling cell faces and corners.

Cases whose lb condition fails (the kernel hands those to the shell search / whole-tree path) are skipped and counted: at
most 5 % of a generator's cases.  The point sets hold two nodes per cell on average, so the nearest node is almost always
within a cell's width."""
import numpy as np
import pytest

F32 = np.float32
MAX_SKIPPED = 0.05


def f32_up(x):
    """lane_query_common.hpp: a binary32 value >= x (two ulps of slack)"""
    t = F32(x)
    return F32(t + F32(abs(t)) * F32(2.0 ** -22) + F32(1e-37))


def fma32(a, b, c):
    """binary32 fused multiply-add of binary32 arrays (the product of two binary32 values is exact in binary64; the one
    binary64 addition in front of the final rounding is exact for the cell-sized operands used here)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


class Grid:
    """cells_build / cell_place for nodes in the box [0, width]^D cut into G cells along every axis"""

    def __init__(self, nodes, G, width):
        self.nodes = np.asarray(nodes, dtype=np.float64)
        self.dim = self.nodes.shape[1]
        self.G = G
        self.inv_h = G / width
        t = self.nodes * self.inv_h                       # lo = 0
        fl = np.floor(t)
        self.ci = np.where(fl > 0.0, np.where(fl < G, fl, G - 1.0), 0.0)
        fr = (t - self.ci) * 65536.0
        self.ui = np.where(fr > 0.0, np.where(fr < 65535.0, np.floor(fr), 65535.0), 0.0)
        dec = self.ci + (self.ui + 0.5) * 2.0 ** -16
        derr = float(np.abs(dec - t).max())
        self.delta_node = float(f32_up(derr * (1.0 + 1e-9) + 1e-30))
        self.A = np.sqrt(float(self.dim)) * (self.delta_node + (G + 8) * 2.0 ** -23) * 1.01 + 1e-30

    def place_query(self, q):
        tq = ((np.asarray(q, dtype=np.float64)) * self.inv_h).astype(F32)
        fl = np.floor(tq)
        cq = np.where(fl > 0, np.where(fl < F32(self.G), fl, F32(self.G - 1)), F32(0)).astype(np.int64)
        return tq, cq

    def screen(self, tq, idx):
        """block_eval's binary32 squared distance (cell units) of the nodes idx from the query at tq"""
        s = None
        for k in range(self.dim):
            off = F32(F32(self.ci[idx, k].astype(F32)) + F32(2.0 ** -17)) - tq[k]
            e = fma32(self.ui[idx, k].astype(F32), np.full(idx.shape, 2.0 ** -16, dtype=F32), off.astype(F32))
            s = (e * e).astype(F32) if s is None else fma32(e, e, s)
        return s

    def block_lb(self, tq, cq):
        """block_lb(grid, tq, cq, 1): distance to the nearest open face of the 3^D block"""
        lb = np.inf
        for k in range(self.dim):
            if cq[k] > 1:
                lb = min(lb, float(tq[k]) - float(cq[k] - 1))
            if cq[k] + 2 < self.G:
                lb = min(lb, float(cq[k] + 2) - float(tq[k]))
        return lb

    def band(self, q):
        """the node indices cells_band_resolve lists for the query, or None when it declines for the lb condition"""
        tq, cq = self.place_query(q)
        d = self.ci.astype(np.int64) - cq
        in_block = np.flatnonzero((np.abs(d) <= 1).all(axis=1))
        if in_block.size == 0:
            return None
        s = self.screen(tq, in_block)
        s1 = s.min()
        B = np.sqrt(float(s1)) * (1.0 + 2.0 ** -20) + 2.0 * self.A
        if not B < self.block_lb(tq, cq) * (1.0 - 2.0 ** -20):
            return None
        thr2 = f32_up(B * B * (1.0 + 2.0 ** -20))
        # the cells the lanes take: squared box gap <= thr2 (gaps scaled down by 2^-20, summed in binary32)
        gap2 = np.zeros(in_block.size, dtype=F32)
        for k in range(self.dim):
            lo = F32(max(F32(tq[k] - F32(cq[k])), F32(0.0)) * F32(1.0 - 2.0 ** -20))
            hi = F32(max(F32(F32(cq[k] + 1) - tq[k]), F32(0.0)) * F32(1.0 - 2.0 ** -20))
            dk = d[in_block, k]
            gk = np.where(dk < 0, lo, hi).astype(F32)
            gap2 = np.where(dk != 0, (gap2 + gk * gk).astype(F32), gap2)
        keep = ~(gap2 > thr2) & ~(s > thr2)
        return in_block[keep]


def reference_nearest(nodes, q):
    """rrt.rs:187-196: the first node with the strictly smallest sqrt(sum of squares, in axis order)"""
    d2 = np.zeros(nodes.shape[0])
    for k in range(nodes.shape[1]):
        df = nodes[:, k] - q[k]
        d2 = d2 + df * df
    return int(np.argmin(np.sqrt(d2))), np.sqrt(d2)     # (argmin returns the first minimum)


def check(grid, queries):
    """both claims for every query; returns the number of cases skipped for the lb condition"""
    skipped = 0
    for q in queries:
        want, dist = reference_nearest(grid.nodes, q)
        band = grid.band(q)
        if band is None:
            skipped += 1
            continue
        assert want in band, (q, want)
        order = np.lexsort((band, dist[band]))            # (distance, index), lexicographic
        assert int(band[order[0]]) == want, (q, want, band)
    return skipped


def cloud(rng, dim, G, per_cell=2.0, width=10.0):
    return rng.random((int(per_cell * G ** dim), dim)) * width


@pytest.mark.parametrize("dim,G", [(2, 23), (2, 32), (3, 8), (3, 11)])
def test_band_holds_the_nearest_node_random_sets(dim, G):
    rng = np.random.default_rng(1000 * dim + G)
    grid = Grid(cloud(rng, dim, G), G, 10.0)
    queries = rng.random((1500, dim)) * 10.0
    skipped = check(grid, queries)
    assert skipped <= MAX_SKIPPED * len(queries), skipped


def _with_pair(rng, dim, G, q, n1, n2, clear):
    """a background cloud without the nodes nearer than `clear` to q, and the pair in front (indices 0 and 1)"""
    bg = cloud(rng, dim, G)
    bg = bg[np.sqrt(((bg - q) ** 2).sum(axis=1)) > clear]
    return Grid(np.vstack([n1, n2, bg]), G, 10.0)


def _direction(rng, dim):
    u = rng.normal(size=dim)
    return u / np.sqrt((u * u).sum())


@pytest.mark.parametrize("dim,G", [(2, 32), (3, 11)])
def test_near_ties_at_every_spacing(dim, G):
    """two nodes at distances r and r + eps from the query, eps from 0 to 4A in 64 steps (and the pair swapped, so that the
    farther node holds the lower index), nothing else nearer"""
    rng = np.random.default_rng(77 + dim)
    h = 10.0 / G
    A_world = Grid(cloud(rng, dim, G), G, 10.0).A * h
    cases = skipped = 0
    for step in range(65):
        eps = 4.0 * A_world * step / 64.0
        q = 2.0 * h + rng.random(dim) * (10.0 - 4.0 * h)
        r = (0.05 + 0.3 * rng.random()) * h
        n1 = q + r * _direction(rng, dim)
        n2 = q + (r + eps) * _direction(rng, dim)
        for a, b in ((n1, n2), (n2, n1)):
            skipped += check(_with_pair(rng, dim, G, q, a, b, r + eps + 0.01 * h), [q])
            cases += 1
    assert skipped <= MAX_SKIPPED * cases, (skipped, cases)


@pytest.mark.parametrize("dim,G", [(2, 32), (3, 11)])
def test_exact_ties_keep_the_lower_index(dim, G):
    """mirror images of one offset on a dyadic lattice: bit-identical distances, the lower index wins"""
    rng = np.random.default_rng(5 + dim)
    h = 10.0 / G
    cases = skipped = 0
    for _ in range(40):
        q = np.round((2.0 * h + rng.random(dim) * (10.0 - 4.0 * h)) * 1024.0) / 1024.0
        off = np.round(rng.random(dim) * 0.2 * h * 2.0 ** 20) / 2.0 ** 20 + 2.0 ** -20
        flip = np.ones(dim)
        flip[rng.integers(dim)] = -1.0
        n1, n2 = q + off, q + off * flip
        grid = _with_pair(rng, dim, G, q, n1, n2, float(np.sqrt((off * off).sum())) + 0.01 * h)
        want, dist = reference_nearest(grid.nodes, q)
        assert dist[0] == dist[1] and want == 0
        skipped += check(grid, [q])
        cases += 1
    assert skipped <= MAX_SKIPPED * cases, (skipped, cases)


@pytest.mark.parametrize("dim,G", [(2, 32), (3, 11)])
def test_pairs_straddling_faces_and_corners(dim, G):
    """the query within a few A of a cell face (one axis) or a cell corner (every axis); the pair in the two / the diagonal
    cells that meet there, at distances that differ by 0 .. 4A"""
    rng = np.random.default_rng(31 + dim)
    h = 10.0 / G
    A_world = Grid(cloud(rng, dim, G), G, 10.0).A * h
    cases = skipped = 0
    for corner in (False, True):
        for step in range(33):
            eps = 4.0 * A_world * step / 32.0
            cell = rng.integers(2, G - 2, size=dim)
            q = (cell + rng.random(dim) * 0.8 + 0.1) * h
            axes = range(dim) if corner else [int(rng.integers(dim))]
            side = np.zeros(dim)
            for k in axes:                                    # onto the face / corner, a few A to either side of it
                q[k] = cell[k] * h + (rng.random() - 0.5) * 6.0 * A_world
                side[k] = 1.0
            r = (0.05 + 0.2 * rng.random()) * h
            u = np.abs(_direction(rng, dim)) * np.where(side > 0, 1.0, 0.3)
            u /= np.sqrt((u * u).sum())
            n1 = q + r * u                                    # above the face(s)
            n2 = q - (r + eps) * u * np.where(side > 0, 1.0, -1.0)   # below
            for a, b in ((n1, n2), (n2, n1)):
                skipped += check(_with_pair(rng, dim, G, q, a, b, r + eps + 0.01 * h), [q])
                cases += 1
    assert skipped <= MAX_SKIPPED * cases, (skipped, cases)


def test_model_constants_match_the_kernel_source():
    """the bound, the threshold and the margin the model restates, as the kernel source writes them"""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "oxmpl_amd", "csrc", "rrt_cells.hip")) as f:
        src = f.read()
    body = src.split("cells_band_resolve(")[1].split("\n}\n")[0]
    assert "const double B = sqrt((double)s1) * (1.0 + 0x1p-20) + 2.0 * A;" in body
    assert "if (!(B < block_lb<DIM>(grid, tq, cq, 1u) * (1.0 - 0x1p-20))) return false;" in body
    assert "const float thr2 = f32_up(B * B * (1.0 + 0x1p-20));" in body
    assert "if (total == 0 || total > 64u) return false;" in body
    assert "const double A = sqrt((double)D) * (grid.delta_node + (double)(gmax + 8u) * 0x1p-23) * 1.01 + 1e-30;" in src
