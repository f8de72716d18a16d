"""The host model of a PRM handle's life (DESIGN.md sections 9, 20, 23 and 24): one object that is constructed, planted, re-checked,
grown and pruned in any order, in binary64 and pure Python + numpy.  No GPU, no capi.

Nothing here is a new rule.  Sampling, validity, the motion check and the distances are the golden generators' own primitives
(tests/golden/make_golden.py, make_golden_so3.py), the re-check is make_golden_prm_revalidate.revalidate, pruning and components
are tests/prm_components_shapes.py's host_prune / components, and a grow's edges are tests/prm_grow_helpers.py's expected_growth.
What the model adds is the state that joins them: the states, the ascending rows, n_samples, the sampler's position (stream id and
the ChaCha12Rng object itself, None after planting) and the capacity.  tests/test_prm_lifecycle_model.py pins construct() to the
golden files that already pin the device, and to make_golden_prm*.prm_construct* themselves.

    kind "rn"   R^n, radius rule        obstacles: spheres [(centre, radius)] and boxes [(lo, hi)]
    kind "knn"  R^n, k nearest earlier  the same
    kind "so3"  SO(3), radius rule      obstacles: cones [(centre quaternion, radius)], passed as `spheres`
"""
import os
import sys

import numpy as np

from prm_components_shapes import components as _components, host_prune
from prm_grow_helpers import expected_growth, make_near

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden as mg  # noqa: E402
import make_golden_prm_revalidate as mr  # noqa: E402
import make_golden_so3 as g3  # noqa: E402


class Refusal(Exception):
    """a call the handle refuses: status is the name of the OXHIP_ERR_* code, fragment a piece of its text"""

    def __init__(self, status, fragment):
        Exception.__init__(self, "%s: %s" % (status, fragment))
        self.status, self.fragment = status, fragment


def capacity_of(max_milestones):
    """alloc_prm's rule: the next multiple of 1024"""
    return ((max_milestones + 1023) // 1024) * 1024


def grown_capacity(cap, n_needed):
    """oxhip_prm_grow_roadmap's rule: untouched while n_needed fits; else the next power of two, starting at 1024"""
    if n_needed <= cap:
        return cap
    new = 1024
    while new < n_needed:
        new *= 2
    return new


def default_budget(n):
    """max_samples = 0, for construction (n = max_milestones) and for a grow (n = n_more)"""
    return 4096 * n + (1 << 22)


class HostRoadmap:
    def __init__(self, kind, dim, bounds, connection_radius, max_milestones, knn_k=0, lvs_fraction=0.05, seed=0, stream=0, max_samples=0,
                 spheres=(), boxes=()):
        assert kind in ("rn", "knn", "so3") and (kind == "knn") == bool(knn_k) and (kind != "so3" or dim == 4)
        self.kind, self.dim, self.bounds, self.radius, self.knn_k = kind, dim, bounds, connection_radius, knn_k
        self.fraction, self.seed, self.stream, self.max_milestones, self.max_samples = lvs_fraction, seed, stream, max_milestones, max_samples
        if kind == "so3":
            self.centre, self.max_angle = g3.space_bounds(bounds)
        self.capacity = capacity_of(max_milestones)
        self.states, self.rows, self.n_samples = [], [], 0
        self.rng, self.rng_stream = None, None
        self.set_obstacles(spheres, boxes)

    # ---------------------------------------------------------------------------------------------------- the space's primitives
    def set_obstacles(self, spheres=(), boxes=()):
        self.spheres, self.boxes = [(list(c), float(r)) for c, r in spheres], [(list(lo), list(hi)) for lo, hi in boxes]
        if self.kind == "so3":
            assert not self.boxes
            self.field = g3.Cones(self.spheres)
        else:
            self.field = mg.Field(self.dim, self.spheres, self.boxes)

    def sample(self, rng):
        if self.kind == "so3":
            return g3.sample_uniform(rng, self.centre, self.max_angle)
        return [mg.random_range(rng, lo, hi) for lo, hi in self.bounds]

    def is_valid(self, q):
        return bool(self.field.is_valid(q))

    def check_motion(self, frm, to):
        if self.kind == "so3":
            return bool(g3.check_motion(self.field, self.fraction, frm, to))
        return bool(mg.check_motion(self.field, self.bounds, self.fraction, frm, to))

    def distance(self, a, b):
        return g3.distance(a, b) if self.kind == "so3" else mg.distance(a, b)

    # ---------------------------------------------------------------------------------------------------- what a caller reads
    @property
    def n(self):
        return len(self.states)

    def sizes(self):
        return self.n, sum(len(r) for r in self.rows), self.n_samples

    def states_array(self):
        return np.array(self.states, dtype=np.float64).reshape(self.n, self.dim)

    def csr(self):
        offsets = np.zeros(self.n + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum([len(r) for r in self.rows], dtype=np.uint64)
        return offsets, np.array([v for r in self.rows for v in r], dtype=np.uint32)

    def roadmap(self):
        return (self.states_array(),) + self.csr()

    # ---------------------------------------------------------------------------------------------------- the calls
    def setup(self):
        """clear_roadmap: the roadmap, n_samples and the sampler's position go; the capacity stays"""
        self.states, self.rows, self.n_samples = [], [], 0
        self.rng, self.rng_stream = None, None

    def construct(self):
        """prm.rs:96-154 from word 0 of the configured stream; a roadmap that exists is left alone (prm.rs:106-113)"""
        if self.n:
            return
        self.rng, self.rng_stream, self.n_samples = mg.ChaCha12Rng(self.seed, self.stream), self.stream, 0
        self._extend(self.max_milestones, self.max_samples or default_budget(self.max_milestones), [])

    def plant(self, states, offsets, nbrs):
        s = np.asarray(states, dtype=np.float64).reshape(-1, self.dim)
        off = [int(v) for v in offsets]
        if len(s) > self.max_milestones:
            raise Refusal("CAPACITY", "more milestones than max_milestones")
        assert len(off) == len(s) + 1
        self.states = [[float(v) for v in row] for row in s]
        self.rows = [[int(v) for v in nbrs[off[i]:off[i + 1]]] for i in range(len(s))]
        self.n_samples, self.rng, self.rng_stream = 0, None, None

    def revalidate(self):
        before = self.sizes()[1]
        valid, kept = mr.revalidate(self.states, self.rows, self.is_valid, self.check_motion)
        self.rows = kept
        return np.array(valid, dtype=bool), before - self.sizes()[1]

    def grow(self, n_more, max_samples=0, new_stream=None):
        if n_more == 0:
            raise Refusal("BAD_ARG", "n_more must be at least 1")
        if self.n == 0:
            raise Refusal("UNSAMPLED_STATE_SPACE", "construct_roadmap")
        if new_stream is None and self.rng is None:
            raise Refusal("BAD_ARG", "OXHIP_PRM_GROW_NEW_STREAM")
        live = [self.is_valid(s) for s in self.states]           # once, when the call starts
        if self.knn_k and not all(live):
            raise Refusal("BAD_ARG", "not built")
        self.capacity = grown_capacity(self.capacity, self.n + n_more)
        if new_stream is not None:
            self.rng, self.rng_stream = mg.ChaCha12Rng(self.seed, new_stream), new_stream
        return self._extend(self.n + n_more, max_samples or default_budget(n_more), live)

    def _extend(self, target, budget, live):
        """the reference's loop continued from the held rng: samples until `target` milestones exist or `budget` samples were drawn
        in this call, then the edges of the new milestones [n_old, n_now).  -> (added, drawn)"""
        n_old, drawn = self.n, 0
        while self.n < target and drawn < budget:
            q = self.sample(self.rng)
            drawn += 1
            if self.is_valid(q):
                self.states.append(q)
        self.n_samples += drawn
        if self.n == n_old:
            return 0, drawn
        if self.knn_k:
            self._knn_rows(n_old)
        else:
            near = make_near(self.states, n_old, self.radius, self.distance, so3=self.kind == "so3")
            self.rows = expected_growth(self.rows, self.n, live, near,
                                        lambda pairs: [self.check_motion(self.states[j], self.states[i]) for j, i in pairs])
        return self.n - n_old, drawn

    def _knn_rows(self, n_old):
        """make_golden_prm_knn.prm_construct_knn's selection for the rows [n_old, n_now): the k earlier milestones nearest by
        (distance, index), visited in ascending index order"""
        s = self.states_array()
        self.rows += [[] for _ in range(self.n - n_old)]
        for j in range(n_old, self.n):
            if j == 0:
                continue
            acc = np.zeros(j)
            for k in range(self.dim):
                d = s[j, k] - s[:j, k]
                acc = acc + d * d
            order = np.lexsort((np.arange(j), np.sqrt(acc)))[:min(self.knn_k, j)]
            for i in sorted(int(v) for v in order):
                if self.check_motion(self.states[j], self.states[i]):
                    self.rows[j].append(i)
                    self.rows[i].append(j)

    def prune(self, invalid=False, keep=None, min_size=0, largest=False):
        """-> (new_index, n_kept, removed entries); n_samples, the sampler's position and the capacity stay"""
        if not (invalid or keep is not None or min_size or largest):
            raise Refusal("BAD_ARG", "flags must name at least one")
        stage1 = np.ones(self.n, dtype=bool)
        if invalid:
            stage1 &= np.array([self.is_valid(s) for s in self.states], dtype=bool)
        if keep is not None:
            stage1 &= np.asarray(keep).reshape(self.n) != 0
        offsets, nbrs = self.csr()
        try:
            out = host_prune(self.states_array(), offsets, nbrs, stage1, min_size, largest)
        except ValueError:
            raise Refusal("BAD_ARG", "would keep no milestone")
        off = [int(v) for v in out["offsets"]]
        self.states = [[float(v) for v in row] for row in out["states"]]
        self.rows = [[int(v) for v in out["nbrs"][off[i]:off[i + 1]]] for i in range(out["n_kept"])]
        return out["new_index"], out["n_kept"], out["n_removed_entries"]

    def components(self):
        """(label, size, n_components, largest_label, largest_size)"""
        offsets, nbrs = self.csr()
        return _components(self.n, offsets, nbrs)
