"""Mirror of `oxmpl_py.geometric` (reference: oxmpl-py/src/geometric/rrt.rs:30-136) for the GPU path.

    planner = RRT(max_distance=0.5, goal_bias=0.05, problem_definition=problem_def)
    planner.setup(SphereBoxValidityChecker(...))
    path = planner.solve(timeout_secs=5.0)      # -> Path; raises Exception(str) like the reference

`RRTBatch` (oxmpl_amd.capi) is the batched form the benchmark uses; this class is the one-problem
drop-in for users of the reference's Python API.
"""
import collections
import contextlib

import numpy as np

from . import capi
from .base import (Path, ProblemDefinition, RealVectorState, RealVectorStateSpace, SE3RigidBodyValidityChecker, SE3State,
                   SE3StateSpace, SO2ArcValidityChecker, SO2State, SO2StateSpace, SO3ConeValidityChecker, SO3State, SO3StateSpace,
                   SphereBoxValidityChecker)

_MESSAGES = {  # Display strings of PlanningError (oxmpl/src/base/error.rs:110-136)
    capi.ERR_TIMEOUT: "No solution found within timeout.",
    capi.ERR_NO_SOLUTION_FOUND: "No solution found.",
    capi.ERR_PLANNER_UNINITIALISED: "<Planner>.setup() was not called, thus Planner is uninitialised.",
    capi.ERR_INVALID_START_STATE: "Start state is not valid in the current StateSpace.",
    capi.ERR_UNSAMPLED_STATE_SPACE: "StateSpace is not sampled. Either Tree or Roadmap is empty.",
}
# statuses that are the caller's ValueError: a space the library refuses to create; an argument a roadmap call refuses
_AT_CREATE = (capi.ERR_UNBOUNDED, capi.ERR_ZERO_VOLUME, capi.ERR_BAD_ARG)
_REFUSED_ARGUMENT = (capi.ERR_BAD_ARG, capi.ERR_CAPACITY)


def _ready(handle):
    """a planner's library handle if setup() has made one, else the reference's PlannerUninitialised"""
    if handle is None:
        raise Exception(_MESSAGES[capi.ERR_PLANNER_UNINITIALISED])
    return handle


@contextlib.contextmanager
def _translated(value_errors=(), messages=True):
    """A capi.OxhipError raised inside becomes ValueError when its status is one of `value_errors`, the reference-style
    Exception(message) when `messages` and the status is a PlanningError's; any other passes as it is."""
    try:
        yield
    except capi.OxhipError as e:
        if e.status in value_errors:
            raise ValueError(str(e)) from None
        if messages and e.status in _MESSAGES:
            raise Exception(_MESSAGES[e.status]) from None
        raise


# ---- the state spaces of the GPU path, one row each.  A state's width in the C ABI is its space's `dimension`.

def _pairs(items):
    """[(a, b), ...] -> ([a, ...], [b, ...]): the two arguments of a handle's set_spheres / set_boxes / set_body"""
    return [a for a, _ in items], [b for _, b in items]


# upload(handle, checker, clear): the checker's obstacles to an RRTBatch or a PRMRoadmap.  setup() leaves an empty list out
# (a new handle has no obstacles); revalidate() passes clear=True, because an empty list must clear the old ones.
def _upload_real_vector(handle, checker, clear):
    if clear or checker.spheres:
        handle.set_spheres(*_pairs(checker.spheres))
    if clear or checker.boxes:
        handle.set_boxes(*_pairs(checker.boxes))


def _upload_so2(handle, checker, clear):
    handle.set_boxes([[lo] for lo, _ in checker.arcs], [[hi] for _, hi in checker.arcs])


def _upload_so3(handle, checker, clear):
    if clear or checker.cones:
        handle.set_spheres(*_pairs(checker.cones))


def _upload_se3(handle, checker, clear):
    handle.set_body(*_pairs(checker.body))
    if clear or checker.obstacles:
        handle.set_spheres(*_pairs(checker.obstacles))


def _so2_state(row):
    s = SO2State(0.0)
    s.value = float(row[0])   # a tree's states are stored as the planner made them: no second normalisation
    return s


_TREE_PLANNERS = (capi.PLANNER_RRT, capi.PLANNER_RRT_CONNECT, capi.PLANNER_RRT_STAR)
_Space = collections.namedtuple("_Space", [
    "cls",        # the space class of oxmpl_amd.base
    "kind",       # capi.SPACE_*
    "bounds",     # space -> the config's bounds as the C ABI reads them for this kind
    "planners",   # the capi.PLANNER_* it is built for,
    "prm",        # ... whether PRM takes it,
    "refusal",    # ... and what every other planner answers
    "checker",    # the validity checker class it accepts
    "describe",   # what that checker describes, for setup()'s refusal of any other object
    "recheck",    # revalidate()'s refusal of any other object; {} is "tree" or "roadmap"
    "upload",     # (handle, checker, clear): the checker's obstacles to the device
    "state",      # device row -> state object
    "file_name",  # the space's name in a save_roadmap file
])
_SPACES = (
    _Space(RealVectorStateSpace, capi.SPACE_REAL_VECTOR, lambda space: space.bounds, _TREE_PLANNERS, True, None,
           SphereBoxValidityChecker, "the obstacles", "describe the obstacles with oxmpl_amd.base.SphereBoxValidityChecker",
           _upload_real_vector, RealVectorState, "real_vector"),
    _Space(SO2StateSpace, capi.SPACE_SO2, lambda space: space.config_bounds(), (capi.PLANNER_RRT,), False,
           "SO(2) is built for RRT only", SO2ArcValidityChecker, "the forbidden arcs",
           "an SO(2) {} is re-checked against an SO2ArcValidityChecker", _upload_so2, _so2_state, "so2"),
    _Space(SO3StateSpace, capi.SPACE_SO3, lambda space: space.config_bounds(), (capi.PLANNER_RRT,), True,
           "SO(3) is built for RRT only", SO3ConeValidityChecker, "the forbidden cones",
           "an SO(3) {} is re-checked against an SO3ConeValidityChecker", _upload_so3, lambda row: SO3State(*row), "so3"),
    _Space(SE3StateSpace, capi.SPACE_SE3, lambda space: space.config_bounds(), (capi.PLANNER_RRT_CONNECT,), False,
           "SE(3) is built for RRTConnect only", SE3RigidBodyValidityChecker, "the body and the obstacles",
           "an SE(3) {} is re-checked against an SE3RigidBodyValidityChecker", _upload_se3, SE3State.from_values, "se3"),
)


def _row(space):
    for row in _SPACES:
        if isinstance(space, row.cls):
            return row
    raise TypeError("no GPU planner is built for %s" % type(space).__name__)


def _set_up(previous, row, pd, checker, create):
    """setup() after the planner's own refusal: refuse the checker, close the planner's previous handle, create() the new
    one, upload the obstacles, hand the problem to the library -> the new handle.  A refusal leaves `previous` open."""
    if not isinstance(checker, row.checker):
        raise TypeError("the GPU path cannot call a Python function per interpolated state; "
                        "describe %s with oxmpl_amd.base.%s" % (row.describe, row.checker.__name__))
    if previous is not None:
        previous.close()
    with _translated(_AT_CREATE, messages=False):
        handle = create()
    row.upload(handle, checker, False)
    handle.setup(pd.start_state.values, pd.goal.target.values, float(pd.goal.radius))
    return handle


def _new_obstacles(handle, space, checker, what):
    """revalidate(checker): the checker's obstacles replace the ones `handle` has (`what`: "tree" or "roadmap")"""
    row = _row(space)
    if not isinstance(checker, row.checker):
        raise TypeError(row.recheck.format(what))
    row.upload(handle, checker, True)


def _path(space, rows):
    state = _row(space).state
    return Path([state(row) for row in rows])


class RRT:
    """One-problem drop-in for `oxmpl_py.geometric.RRT`.

    Difference from the reference, on purpose: the tree lives in a device buffer sized at setup(), so it is capped at
    `max_nodes` (default 10,000).  The reference has no node cap (rrt.rs:170-226 grows until the wall clock runs out);
    here a problem that fills its tree before the timeout ends with "No solution found." (PlanningError::NoSolutionFound,
    declared but unused by the reference's RRT) instead of "No solution found within timeout.".  Pass a larger `max_nodes`
    for narrow-passage problems.  `solve(0)` is Timeout, as upstream."""
    _PLANNER = capi.PLANNER_RRT
    search_radius = 0.0   # (means something to RRTStar only)

    def __init__(self, max_distance, goal_bias, problem_definition, max_nodes=10000, seed=0, problem_id=0, device=0,
                 goal_sampler=capi.GOAL_SAMPLE_CENTRE):
        """goal_sampler: what `goal.sample_goal()` draws on the device -- capi.GOAL_SAMPLE_CENTRE (the goal's `target`, as the
        README's goal, no random draw) or capi.GOAL_SAMPLE_UNIFORM_DISC (uniform in the disc as the CircularGoal of
        oxmpl-py/tests/test_rrt_rvss.py:19-25 and oxmpl/tests/rrt_rvss_tests.rs:55-66 samples it; 2-D spaces)"""
        if not isinstance(problem_definition, ProblemDefinition):
            raise TypeError("problem_definition must be a ProblemDefinition")
        self.max_distance, self.goal_bias = float(max_distance), float(goal_bias)
        self._pd = problem_definition
        self._opts = dict(max_nodes=max_nodes, seed=seed, first_problem_id=problem_id, device=device, goal_sampler=goal_sampler)
        self._batch = None

    def setup(self, validity_checker):
        """Planner::setup (rrt.rs:140-156).  The reference takes a Python callable here; the GPU path
        takes a SphereBoxValidityChecker (see oxmpl_amd.base), or an SO3ConeValidityChecker for an SO(3) problem (RRT only),
        or an SO2ArcValidityChecker for an SO(2) problem (RRT only), or an SE3RigidBodyValidityChecker for an SE(3) problem
        (RRTConnect only)."""
        pd = self._pd
        row = _row(pd.space)
        if self._PLANNER not in row.planners:
            raise TypeError(row.refusal)
        self._batch = _set_up(self._batch, row, pd, validity_checker, lambda: capi.RRTBatch(
            pd.space.dimension, row.bounds(pd.space), self.max_distance, self.goal_bias, 1,
            lvs_fraction=pd.space.longest_valid_segment_fraction, stop_at_goal=True, planner=self._PLANNER,
            search_radius=self.search_radius, space=row.kind, **self._opts))
        self._checker = validity_checker

    def solve(self, timeout_secs):
        """Planner::solve (rrt.rs:158-227); errors surface as Exception(message) like the reference
        (oxmpl-py/src/geometric/rrt.rs:117)."""
        batch = _ready(self._batch)
        timeout_secs = float(timeout_secs)
        if timeout_secs != timeout_secs or timeout_secs < 0.0:
            # Duration::from_secs_f32 (oxmpl-py/src/geometric/rrt.rs:111) panics on NaN / negative values
            raise ValueError("timeout_secs must be a non-negative number")
        if timeout_secs == 0.0:
            # rrt.rs:172-174: `start_time.elapsed() > timeout` already holds at the first check
            raise Exception(_MESSAGES[capi.ERR_TIMEOUT])
        st = batch.solve(1 << 40, timeout_s=timeout_secs)
        if st[0] != capi.OK:
            raise Exception(_MESSAGES.get(int(st[0]), capi.status_string(int(st[0]))))
        return _path(self._pd.space, batch.path(0))

    def simplify_solution(self, max_span=0):
        """The last solution, shortcut over its own waypoints on the device (the cheapest chain of
        waypoints whose links pass the planner's own check_motion; `max_span` bounds how many waypoints a link may skip over,
        0 = no bound) -> Path.  Not part of the reference's surface.  Raises the reference-style Exception when there is no
        solution, TypeError on SE(3), for which the shortcut is not built."""
        batch = _ready(self._batch)
        if _row(self._pd.space).kind == capi.SPACE_SE3:
            raise TypeError("simplify_solution is not built for SE(3)")
        if int(batch.counts()["goal_node"][0]) < 0:
            raise Exception(_MESSAGES[capi.ERR_NO_SOLUTION_FOUND])
        batch.simplify_paths(int(max_span))
        return _path(self._pd.space, batch.simplified_paths()[1])

    def is_state_valid(self, state):
        """the checker's predicate, evaluated on the device (the reference calls the user's callable)"""
        return bool(self._batch.is_valid(np.array([state.values]))[0])

    def revalidate(self, validity_checker=None):
        """Re-checks every edge of the tree against the obstacles as they are now -- `validity_checker`'s when one is given (it
        replaces the planner's), else the ones already set -- and drops every node that a failed edge cuts off from the start
        (DESIGN.md section 21).  Returns the number of removed nodes; a later solve() continues from the pruned tree, with the
        counters and the random stream where they were.  Not part of the reference's surface.  RRT only."""
        if self._PLANNER != capi.PLANNER_RRT:
            raise TypeError("revalidate is built for RRT only (not RRTConnect, not RRTStar)")
        batch = _ready(self._batch)
        if validity_checker is not None:
            _new_obstacles(batch, self._pd.space, validity_checker, "tree")
            self._checker = validity_checker
        with _translated():
            return int(batch.revalidate_trees()["n_removed"][0])

    @property
    def num_nodes(self):
        return int(self._batch.counts()["nodes"][0])


class RRTConnect(RRT):
    """oxmpl_py.geometric.RRTConnect (oxmpl-py/src/geometric/rrt_connect.rs; planner:
    oxmpl/src/geometric/planners/rrt_connect.rs): same constructor / setup / solve surface as RRT,
    two trees grown towards each other; `max_nodes` caps each tree."""
    _PLANNER = capi.PLANNER_RRT_CONNECT

    @property
    def num_nodes(self):
        return int(self._batch.counts()["nodes"][0]) + int(self._batch.goal_counts()["nodes"][0])


class RRTStar(RRT):
    """oxmpl_py.geometric.RRTStar (oxmpl-py/src/geometric/rrt_star.rs:30-140; planner:
    oxmpl/src/geometric/planners/rrt_star.rs): RRTStar(max_distance, goal_bias, search_radius, problem_definition)."""
    _PLANNER = capi.PLANNER_RRT_STAR

    def __init__(self, max_distance, goal_bias, search_radius, problem_definition, **opts):
        super().__init__(max_distance, goal_bias, problem_definition, **opts)
        self.search_radius = float(search_radius)

    def path_cost(self):
        """Node::cost of the goal node (rrt_star.rs:26)"""
        g = int(self._batch.counts()["goal_node"][0])
        return float(self._batch.costs(0)[g]) if g >= 0 else float("inf")


class PRM:
    """oxmpl_py.geometric.PRM (oxmpl-py/src/geometric/prm.rs:30-206; planner: oxmpl/src/geometric/planners/prm.rs).

        planner = PRM(timeout=5.0, connection_radius=0.5, problem_definition=problem_def)
        planner.setup(SphereBoxValidityChecker(...))
        planner.construct_roadmap()
        path = planner.solve(timeout_secs=5.0)

    The reference samples for `timeout` seconds of wall clock; the device path also stops at `max_milestones`
    (a GPU fills five seconds with tens of millions of milestones).  `seed` / `stream` key the sampler."""

    def __init__(self, timeout, connection_radius, problem_definition, max_milestones=16384, max_samples=0, seed=0,
                 stream=0, device=0):
        if not isinstance(problem_definition, ProblemDefinition):
            raise TypeError("problem_definition must be a ProblemDefinition")
        self.timeout, self.connection_radius = float(timeout), float(connection_radius)
        self._pd = problem_definition
        self._opts = dict(max_milestones=max_milestones, max_samples=max_samples, seed=seed, stream=stream, device=device)
        self._prm = None

    def setup(self, validity_checker):
        """Planner::setup (prm.rs:217-225): stores problem and checker, clears the roadmap.  An SO(3) problem takes an
        SO3ConeValidityChecker (the radius rule; milestones and path states are SO3State).  SO(2) is built for RRT only,
        SE(3) for RRTConnect only."""
        pd = self._pd
        row = _row(pd.space)
        if not row.prm:
            raise TypeError(row.refusal)
        self._prm = _set_up(self._prm, row, pd, validity_checker, lambda: capi.PRMRoadmap(
            pd.space.dimension, row.bounds(pd.space), self.connection_radius, timeout=self.timeout,
            lvs_fraction=pd.space.longest_valid_segment_fraction, space=row.kind, **self._opts))

    def set_problem_definition(self, problem_definition):
        """PRM::set_problem_definition (prm.rs:88-90): new start / goal on the roadmap already built"""
        if not isinstance(problem_definition, ProblemDefinition):
            raise TypeError("problem_definition must be a ProblemDefinition")
        self._pd = problem_definition
        if self._prm is not None:
            self._prm.set_problem(problem_definition.start_state.values, problem_definition.goal.target.values,
                                  float(problem_definition.goal.radius))

    def construct_roadmap(self):
        _ready(self._prm).construct_roadmap()

    def solve(self, timeout_secs):
        """Planner::solve (prm.rs:227-307); errors surface as Exception(message) like the reference
        (oxmpl-py/src/geometric/prm.rs:120-145)"""
        st, path = _ready(self._prm).solve(float(timeout_secs))
        if st != capi.OK:
            raise Exception(_MESSAGES.get(int(st), capi.status_string(int(st))))
        return _path(self._pd.space, path)

    def solve_batch(self, problem_definitions, timeout_secs, shortest=False):
        """Many problem definitions on the roadmap already built, in one device call (oxhip_prm_solve_batch: start
        connections, goal test, breadth-first search and path extraction on the GPU).  Returns a list with, per problem, what
        set_problem_definition + solve would give: a Path, or an Exception instance carrying the reference's message for that
        status -- returned, not raised, so one start in collision does not hide a thousand answers.  The planner's own problem
        definition is left as it is.  All problems must share the planner's space.  shortest=True answers every problem with
        a shortest path on the roadmap in the space's distance (oxhip_prm_solve_batch_shortest) instead of the reference's
        fewest-hop path; the statuses are the same."""
        prm = _ready(self._prm)
        pds = list(problem_definitions)
        for pd in pds:
            if not isinstance(pd, ProblemDefinition):
                raise TypeError("problem_definitions must hold ProblemDefinition objects")
            if type(pd.space) is not type(self._pd.space) or len(pd.start_state.values) != len(self._pd.start_state.values):
                raise ValueError("every problem of a batch must share the planner's state space")
        with _translated():
            run = prm.solve_batch_shortest if shortest else prm.solve_batch
            status = run([pd.start_state.values for pd in pds], [pd.goal.target.values for pd in pds],
                         [float(pd.goal.radius) for pd in pds], float(timeout_secs))
        offsets, _, rows = prm.batch_paths()
        out = []
        for q, st in enumerate(status):
            if st != capi.OK:
                out.append(Exception(_MESSAGES.get(int(st), capi.status_string(int(st)))))
            else:
                out.append(_path(self._pd.space, rows[int(offsets[q]):int(offsets[q + 1])]))
        return out

    def simplify_batch(self, subdivide=1, max_span=0):
        """The answered paths of the last solve_batch, shortcut on the device (oxhip_prm_batch_simplify_paths, DESIGN.md
        section 25): every edge is first cut into `subdivide` equal parts, so a link may leave and join the path between its
        milestones, and the cheapest chain of the resulting points whose links pass the planner's own check_motion is
        returned; `max_span` bounds how many original edges a link may span, 0 = no bound.  Returns a list with a Path per
        answered problem and None for every other one.  Not part of the reference's surface.  ValueError for a refused
        argument or a path too large for the device's pair matrix; the reference-style Exception when no batch was solved."""
        prm = _ready(self._prm)
        with _translated(_REFUSED_ARGUMENT):
            prm.simplify_batch_paths(int(subdivide), int(max_span))
            offsets, rows, _ = prm.simplified_batch_paths()
        return [_path(self._pd.space, rows[int(a):int(b)]) if b > a else None for a, b in zip(offsets[:-1], offsets[1:])]

    def simplify_solution(self, subdivide=1, max_span=0):
        """The planner's own problem definition answered and shortcut: it runs that query as a one-query batch, which
        replaces "the last batch" (a solve_batch's paths are gone afterwards), and shortcuts it as simplify_batch does
        -> Path.  Raises the reference-style Exception when the query has no solution."""
        prm = _ready(self._prm)
        pd = self._pd
        with _translated():
            status = prm.solve_batch([pd.start_state.values], [pd.goal.target.values], [float(pd.goal.radius)])
        if status[0] != capi.OK:
            raise Exception(_MESSAGES.get(int(status[0]), capi.status_string(int(status[0]))))
        return self.simplify_batch(subdivide, max_span)[0]

    def get_roadmap(self):
        """PRM::get_roadmap (prm.rs:82-84) as (states, offsets, neighbours): node i's edges are
        neighbours[offsets[i]:offsets[i+1]].  SO(3) problems: states is a list of SO3State; a real-vector roadmap's states
        stay the [n][dim] array."""
        states, offsets, nbrs = self._prm.roadmap()
        row = _row(self._pd.space)
        if row.kind != capi.SPACE_REAL_VECTOR:
            states = [row.state(r) for r in states]
        return states, offsets, nbrs

    # ---- a roadmap that outlives its planner, and one that follows its scene (oxhip_prm_set_roadmap / oxhip_prm_revalidate)

    def set_roadmap(self, states, offsets, neighbours):
        """Replaces the roadmap with the caller's, in the layout get_roadmap returns (states: rows or state objects).  The
        library checks the structure on the GPU and raises ValueError, naming the rule and the lowest offending row, when it is
        not a symmetric roadmap with ascending rows; the planner's roadmap is then unchanged."""
        prm = _ready(self._prm)
        rows = [s.values if hasattr(s, "values") else s for s in states]
        with _translated(_REFUSED_ARGUMENT, messages=False):
            prm.set_roadmap(rows, offsets, neighbours)

    def revalidate(self, validity_checker=None):
        """Re-checks every milestone and edge of the roadmap against the obstacles as they are now -- `validity_checker`'s when
        one is given (it replaces the planner's), else the ones already set.  Milestone indices are stable: an invalid
        milestone keeps its place and loses its edges.  Returns (valid_mask [n] bool, removed edge entries)."""
        prm = _ready(self._prm)
        if validity_checker is not None:
            _new_obstacles(prm, self._pd.space, validity_checker, "roadmap")
        with _translated():
            return prm.revalidate()

    def grow_roadmap(self, n_more, max_samples=0, new_stream=None):
        """Adds up to n_more milestones to the roadmap as it stands -- built, loaded or re-checked -- under the obstacles as they
        are now (oxhip_prm_grow_roadmap; OMPL's PRM::growRoadmap).  Old indices and rows stay; a milestone that is invalid now
        gets no new edge.  new_stream=None continues the planner's own sampler where construct_roadmap or the last grow
        stopped; a loaded roadmap has no such position and needs new_stream=<stream id>.  ValueError for a refused argument or
        too many milestones.  Returns (milestones added, samples drawn)."""
        prm = _ready(self._prm)
        with _translated(_REFUSED_ARGUMENT):
            return prm.grow(int(n_more), int(max_samples), None if new_stream is None else int(new_stream))

    def components(self):
        """The roadmap's connected components (oxhip_prm_components): (label [n], size [n], n_components, largest_label,
        largest_size), label[i] being the lowest milestone index of i's component.  Two milestones can be joined by a path
        on the roadmap iff their labels are equal."""
        prm = _ready(self._prm)
        with _translated():
            return prm.components()

    def prune_roadmap(self, invalid=False, keep=None, min_size=0, largest=False):
        """Removes milestones from the roadmap and renumbers the rest in their old order (oxhip_prm_prune): first the ones that
        are invalid now (invalid=True) and the ones keep[i] is false for, then -- on the components of what is left --
        components below min_size milestones and, with largest=True, all but the largest component.  No edge is re-checked.
        ValueError for a refused argument or a call that would keep no milestone.  Returns (new_index [n before] with -1 =
        dropped, milestones kept, edge entries removed)."""
        prm = _ready(self._prm)
        with _translated(_REFUSED_ARGUMENT):
            return prm.prune(bool(invalid), keep, int(min_size), bool(largest))

    def save_roadmap(self, path):
        """The roadmap as a .npz file: states, offsets, neighbours, the space's kind and the width of a state."""
        states, offsets, nbrs = _ready(self._prm).roadmap()
        with open(path, "wb") as f:
            np.savez(f, states=states, offsets=offsets, neighbours=nbrs, space=np.array(_row(self._pd.space).file_name),
                     dim=np.array(int(self._pd.space.dimension), dtype=np.uint32))

    def load_roadmap(self, path):
        """Plants the roadmap of a save_roadmap file.  ValueError -- before any device call -- when the file's space or
        dimension is not the planner's."""
        with np.load(path, allow_pickle=False) as z:
            space, dim = str(z["space"]), int(z["dim"])
            states, offsets, nbrs = z["states"], z["offsets"], z["neighbours"]
        own = (_row(self._pd.space).file_name, int(self._pd.space.dimension))
        if (space, dim) != own:
            raise ValueError("roadmap file is for %s dim %d, the planner's space is %s dim %d" % ((space, dim) + own))
        if states.ndim != 2 or states.shape[1] != dim or offsets.shape != (states.shape[0] + 1,):
            raise ValueError("roadmap file is malformed: states %s, offsets %s" % (states.shape, offsets.shape))
        self.set_roadmap(states, offsets, nbrs)

    @property
    def num_milestones(self):
        return 0 if self._prm is None else self._prm.sizes()[0]
