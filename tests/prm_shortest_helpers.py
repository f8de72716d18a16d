"""Test-side helpers of the shortest-path PRM batch tests (test_gpu_prm_shortest.py, test_gpu_prm_shortest_shapes.py): a roadmap on
the device, a batch with everything its getters return, and the pure-Python checker (tests/golden/make_golden_prm_shortest.py) fed
with the device's own roadmap and query sets."""
import os
import sys

import numpy as np

from helpers import bits, params_spheres, params_boxes
from prm_helpers import STATUS_NAME

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_prm_shortest as gsp  # noqa: E402

from oxmpl_amd import capi  # noqa: E402

START_ROW = 0xFFFFFFFF
DISTANCE, UNIT, ZERO = 0, 1, 2


def make_gpu_prm(P, **kw):
    args = dict(max_milestones=P["max_milestones"], lvs_fraction=P["fraction"], seed=P["seed"], stream=P["stream"],
                max_samples=0 if P["max_samples"] >= 10 ** 9 else P["max_samples"])
    args.update(kw)
    g = capi.PRMRoadmap(P["dim"], P["bounds"], P["radius"], **args)
    if P["spheres"]:
        g.set_spheres(*params_spheres(P))
    if P["boxes"]:
        g.set_boxes(*params_boxes(P))
    return g


class Batch:
    """one batch -- shortest paths with `weights`, or the breadth-first one (weights=None) -- and everything its getters return"""

    def __init__(self, g, starts, goals, radii, weights=DISTANCE, **kw):
        self.starts = np.asarray(starts, dtype=np.float64).reshape(len(radii), g.dim)
        if weights is None:
            self.status = g.solve_batch(starts, goals, radii, **kw).copy()
        else:
            self.status = g.solve_batch_shortest(starts, goals, radii, weights=weights, **kw).copy()
        r = g.batch_results()
        assert np.array_equal(self.status, r["status"])
        self.len, self.goal, self.ns, self.ng = r["path_len"], r["goal_node"], r["n_start"], r["n_goal"]
        self.off, self.nodes, self.rows = g.batch_paths()
        self.timing = g.batch_last_timing()
        self.cost = None if weights is None else g.batch_costs().copy()
        q = len(radii)
        assert len(self.status) == q and len(self.off) == q + 1 and int(self.off[0]) == 0
        assert np.array_equal(np.diff(self.off.astype(np.int64)), self.len.astype(np.int64))
        assert len(self.nodes) == int(self.off[-1]) and self.rows.shape == (int(self.off[-1]), g.dim)
        ok = self.status == capi.OK
        assert np.all(self.len[~ok] == 0) and np.all(self.goal[~ok] == -1) and np.all(self.len[ok] >= 2)
        bad = (self.status == capi.ERR_INVALID_START_STATE) | (self.status == capi.ERR_TIMEOUT)
        assert np.all(self.ns[bad] == 0) and np.all(self.ng[bad] == 0)
        assert set(np.unique(self.status)) <= {capi.OK, capi.ERR_NO_SOLUTION_FOUND, capi.ERR_INVALID_START_STATE, capi.ERR_TIMEOUT}
        if self.cost is not None:
            assert np.all(np.isinf(self.cost[~ok])) and np.all(np.isfinite(self.cost[ok]))

    def path(self, q):
        return self.rows[int(self.off[q]):int(self.off[q + 1])]

    def path_nodes(self, q):
        return [int(v) for v in self.nodes[int(self.off[q]):int(self.off[q + 1])]]

    def check_rows_are_milestones(self, milestones):
        for q in np.nonzero(self.status == capi.OK)[0]:
            nd, rows = self.path_nodes(q), self.path(q)
            assert nd[0] == START_ROW and np.array_equal(bits(rows[0]), bits(self.starts[q]))
            assert np.array_equal(bits(rows[1:]), bits(milestones[nd[1:]]))
            assert nd[-1] == int(self.goal[q])

    def same_as(self, other, upto=None):
        n = len(self.status) if upto is None else upto
        rows = int(other.off[n])
        pairs = [(self.status[:n], other.status[:n]), (self.len[:n], other.len[:n]), (self.goal[:n], other.goal[:n]), (self.ns[:n], other.ns[:n]),
                 (self.ng[:n], other.ng[:n]), (self.off[:n + 1], other.off[:n + 1]), (self.nodes[:rows], other.nodes[:rows]),
                 (bits(self.rows[:rows]), bits(other.rows[:rows]))]
        if self.cost is not None and other.cost is not None:
            pairs.append((bits(self.cost[:n]), bits(other.cost[:n])))
        for a, b in pairs:
            assert np.array_equal(a, b)


class RoadmapChecker:
    """a roadmap on the device (self.g, constructed; self.dist its space's distance), its copy for the checker, and the checker's
    answers from the device's own query sets"""

    def load_roadmap(self):
        self.states, offsets, nbrs = self.g.roadmap()
        self.n = len(offsets) - 1
        self.edges = [[int(v) for v in nbrs[int(offsets[i]):int(offsets[i + 1])]] for i in range(self.n)]
        self.W = {}

    def weights(self, mode):
        if mode not in self.W:
            self.W[mode] = gsp.edge_weights(self.edges, self.states, self.dist, mode)
        return self.W[mode]

    def checker(self, B, q, mode):
        """the checker's answer to query q of batch B, from the device's own roadmap and query sets"""
        sc, gi = self.g.batch_query_sets(q)
        init = gsp.init_labels(self.n, [int(v) for v in sc], [float(v) for v in B.starts[q]], self.states, self.dist, mode)
        return gsp.shortest_query(self.edges, self.weights(mode), init, [int(v) for v in gi])

    def check_against_checker(self, B, mode, queries=None):
        """statuses, costs and node lists of the batch against the checker; -> number solved (self.compared: how many it compared,
        which leaves out the queries with an invalid start)"""
        solved = self.compared = 0
        for q in (range(len(B.status)) if queries is None else queries):
            if B.status[q] == capi.ERR_INVALID_START_STATE:
                continue
            res = self.checker(B, q, mode)
            assert STATUS_NAME[int(B.status[q])] == res["status"], q
            assert bits(np.float64(B.cost[q])) == bits(np.float64(res["cost"])), q
            assert B.path_nodes(q)[1:] == res["nodes"] and int(B.goal[q]) == res["goal"], q
            solved += res["status"] == "solved"
            self.compared += 1
        return solved
