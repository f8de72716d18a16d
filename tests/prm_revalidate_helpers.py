"""Shared by the tests of oxhip_prm_set_roadmap / oxhip_prm_revalidate: the fixture tests/golden/prm_revalidate.json and CSR helpers."""
import json
import os

import numpy as np

from helpers import unhex

HERE = os.path.dirname(os.path.abspath(__file__))
_FIXTURE = None


def fixture():
    global _FIXTURE
    if _FIXTURE is None:
        with open(os.path.join(HERE, "golden", "prm_revalidate.json")) as f:
            _FIXTURE = json.load(f)
    return _FIXTURE


def unhex_rows(rows):
    return np.array([[unhex(v) for v in row] for row in rows], dtype=np.float64)


def valid_mask(scene):
    """the fixture's valid mask (it stores the invalid indices)"""
    valid = np.ones(scene["n"], dtype=bool)
    valid[scene["invalid"]] = False
    return valid


def csr(edge_lists):
    """(offsets u64 [n+1], neighbours u32) of per-node edge lists"""
    offsets = np.zeros(len(edge_lists) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(e) for e in edge_lists], dtype=np.uint64)
    nbrs = np.array([v for e in edge_lists for v in e], dtype=np.uint32)
    return offsets, nbrs


def symmetric_lists(n, pairs):
    """the ascending edge lists of n milestones joined by the undirected pairs (u, v), u != v (a pair named twice counts once)"""
    rows = [set() for _ in range(n)]
    for u, v in pairs:
        assert u != v
        rows[u].add(int(v))
        rows[v].add(int(u))
    return [sorted(r) for r in rows]


def edge_lists(offsets, nbrs):
    return [[int(v) for v in nbrs[int(offsets[i]):int(offsets[i + 1])]] for i in range(len(offsets) - 1)]


def added_spheres(scene):
    """(centres [m][dim], radii [m]) the scene adds (R^n: spheres, SO(3): cones)"""
    rows = scene["added"].get("spheres", scene["added"].get("cones"))
    return unhex_rows([c for c, _ in rows]), np.array([unhex(r) for _, r in rows])


def plain_filter(lists, valid, motion_ok):
    """keep {i < j} iff valid[i], valid[j] and motion_ok[(j, i)]"""
    keep = [[] for _ in lists]
    for j, row in enumerate(lists):
        for i in row:
            if i < j and valid[i] and valid[j] and motion_ok[(j, i)]:
                keep[j].append(i)
                keep[i].append(j)
    return [sorted(r) for r in keep]
