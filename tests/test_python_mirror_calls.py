"""What the Python class surface (oxmpl_amd.geometric over oxmpl_amd.base) asks of the library, call by call.

capi.RRTBatch and capi.PRMRoadmap are replaced by recorders: no library is loaded and no GPU is needed.  Every expectation
below is literal data: which constructor arguments and which uploads a (planner, space, checker) combination produces,
which refusal it gets, which state objects come back from canned device rows, and how a library status turns into an
exception.  A new state space adds its cases to the tables at the top.

Two corners are left open on purpose, because only an accident decided them before the spaces got one table:
  * PRM over SE(3) is refused with a TypeError; which text it carries (and the AttributeError a SphereBoxValidityChecker
    used to run into) is not pinned.
  * ERR_UNBOUNDED from an SO(2) / SO(3) constructor is not pinned: the library raises that status only while it reads
    real-vector bounds (space_resolution in oxhip_host.hpp), which SO(2) and SO(3) configs never reach."""
import inspect
import math

import numpy as np
import pytest

from oxmpl_amd import capi, geometric
from oxmpl_amd.base import (Path, ProblemDefinition, RealVectorState, RealVectorStateSpace, SE3RigidBodyValidityChecker,
                            SE3State, SE3StateSpace, SO2ArcValidityChecker, SO2State, SO2StateSpace, SO3ConeValidityChecker,
                            SO3State, SO3StateSpace, SphereBoxValidityChecker)
from oxmpl_amd.geometric import PRM, RRT, RRTConnect, RRTStar

_REAL = {"RRTBatch": capi.RRTBatch, "PRMRoadmap": capi.PRMRoadmap}
UNINITIALISED = "<Planner>.setup() was not called, thus Planner is uninitialised."


def plain(v):
    """numpy arrays, tuples and numpy scalars as plain lists and numbers"""
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items()}
    return v.item() if isinstance(v, np.generic) else v


class Recorder:
    """Stands in for a capi handle class: logs the constructor's arguments as the real signature binds them (an omitted
    default and an explicit one record alike) and every method call, returns canned results, raises on request."""
    real = None      # the class it replaces
    log = None       # shared by both recorders: [(name, arg, ...)], a trailing dict holding keyword arguments if any
    fail = None      # {method name or "__init__": status}
    canned = None    # {method name: result}

    def __init__(self, *args, **kwargs):
        bound = inspect.signature(self.real.__init__).bind(self, *args, **kwargs)
        bound.apply_defaults()
        a = dict(bound.arguments)
        a.pop("self")
        self.log.append((self.real.__name__, plain(a)))
        self._raise_if_told("__init__")

    def _raise_if_told(self, name):
        if name in self.fail:
            raise capi.OxhipError(self.fail[name], "x")

    def __getattr__(self, name):
        if name.startswith("__") or not hasattr(self.real, name):
            raise AttributeError(name)

        def call(*args, **kwargs):
            self.log.append((name,) + tuple(plain(args)) + ((plain(kwargs),) if kwargs else ()))
            self._raise_if_told(name)
            return self.canned.get(name)
        return call


@pytest.fixture
def rec(monkeypatch):
    """the recorders in place of the two handle classes -> namespace with log / fail / canned"""
    class R:
        log, fail, canned = [], {}, {}
    for name, real in _REAL.items():
        cls = type(name, (Recorder,), dict(real=real, log=R.log, fail=R.fail, canned=R.canned))
        monkeypatch.setattr(capi, name, cls)
        setattr(R, name, cls)
    monkeypatch.setattr(capi, "status_string", lambda status: "status %d" % status)   # OxhipError's text: no library
    return R


def planted(rec, cls_name):
    """a previous handle, as a planner that was set up before holds one"""
    return object.__new__(getattr(rec, cls_name))


class Goal:
    def __init__(self, target, radius):
        self.target, self.radius = target, radius


# ---- the spaces: problem, start / goal rows as setup() hands them on, canned device rows (SO(2): 4.0 is outside [-PI, PI))

def problem(space):
    if space == "r2":
        return ProblemDefinition.from_real_vector(RealVectorStateSpace(2, [(0.0, 10.0), (-1.0, 1.0)]),
                                                  RealVectorState([1.0, 0.0]), Goal(RealVectorState([9.0, 0.5]), 0.5))
    if space == "so2":
        return ProblemDefinition.from_so2(SO2StateSpace((-2.0, 2.5)), SO2State(-1.0), Goal(SO2State(1.5), 0.125))
    if space == "so3":
        return ProblemDefinition.from_so3(SO3StateSpace((SO3State(0.0, 0.0, 0.0, 1.0), 2.0)), SO3State.identity(),
                                          Goal(SO3State(0.0, 0.6, 0.0, 0.8), 0.25))
    return ProblemDefinition.from_se3(SE3StateSpace([(0.0, 1.0), (0.0, 2.0), (0.0, 3.0)]),
                                      SE3State(0.5, 0.5, 0.5, SO3State.identity()),
                                      Goal(SE3State(0.5, 1.5, 2.5, SO3State(0.0, 0.6, 0.0, 0.8)), 0.75))


SPACES = ["r2", "so2", "so3", "se3"]
KIND = {"r2": 0, "so2": 16, "so3": 2, "se3": 3}             # capi.SPACE_*
DIM = {"r2": 2, "so2": 1, "so3": 4, "se3": 7}
BOUNDS = {"r2": [[0.0, 10.0], [-1.0, 1.0]], "so2": [-2.0, 2.5], "so3": [0.0, 0.0, 0.0, 1.0, 2.0],
          "se3": [0.0, 1.0, 0.0, 2.0, 0.0, 3.0, 0.0, 0.0, 0.0, 1.0, math.pi]}
SETUP_CALL = {"r2": ("setup", [1.0, 0.0], [9.0, 0.5], 0.5), "so2": ("setup", [-1.0], [1.5], 0.125),
              "so3": ("setup", [0.0, 0.0, 0.0, 1.0], [0.0, 0.6, 0.0, 0.8], 0.25),
              "se3": ("setup", [0.5, 0.5, 0.5, 0.0, 0.0, 0.0, 1.0], [0.5, 1.5, 2.5, 0.0, 0.6, 0.0, 0.8], 0.75)}
ROWS = {"r2": [[1.0, 0.0], [5.0, 0.25], [9.0, 0.5]], "so2": [[-1.0], [4.0], [1.5]],
        "so3": [[0.0, 0.0, 0.0, 1.0], [0.0, 0.28, 0.0, 0.96], [0.0, 0.6, 0.0, 0.8]],
        "se3": [[0.5, 0.5, 0.5, 0.0, 0.0, 0.0, 1.0], [0.5, 1.0, 1.5, 0.0, 0.28, 0.0, 0.96], [0.5, 1.5, 2.5, 0.0, 0.6, 0.0, 0.8]]}
STATE = {"r2": RealVectorState, "so2": SO2State, "so3": SO3State, "se3": SE3State}

# ---- the checkers: (every list empty, every list non-empty) and the uploads each gives at setup / at revalidate
CHECKERS = {
    "r2": (SphereBoxValidityChecker(), SphereBoxValidityChecker(spheres=[([5.0, 0.0], 0.5)], boxes=[([2.0, -1.0], [3.0, 0.5])])),
    "so2": (SO2ArcValidityChecker(), SO2ArcValidityChecker(arcs=[(0.0, 0.5), (-1.75, -1.5)])),
    "so3": (SO3ConeValidityChecker(), SO3ConeValidityChecker(cones=[(SO3State(0.0, 0.28, 0.0, 0.96), 0.125)])),
    "se3": (SE3RigidBodyValidityChecker(), SE3RigidBodyValidityChecker(body=[([0.0, 0.0, 0.25], 0.125), ([0.0, 0.0, -0.25], 0.0)],
                                                                       obstacles=[([0.5, 1.0, 1.0], 0.25)])),
}
UPLOADS_AT_SETUP = {
    "r2": ([], [("set_spheres", [[5.0, 0.0]], [0.5]), ("set_boxes", [[2.0, -1.0]], [[3.0, 0.5]])]),
    "so2": ([("set_boxes", [], [])], [("set_boxes", [[0.0], [-1.75]], [[0.5], [-1.5]])]),
    "so3": ([], [("set_spheres", [[0.0, 0.28, 0.0, 0.96]], [0.125])]),
    "se3": ([("set_body", [[0.0, 0.0, 0.0]], [0.0])],
            [("set_body", [[0.0, 0.0, 0.25], [0.0, 0.0, -0.25]], [0.125, 0.0]), ("set_spheres", [[0.5, 1.0, 1.0]], [0.25])]),
}
UPLOADS_AT_REVALIDATE = {   # an empty list is uploaded too: it clears the old obstacles
    "r2": ([("set_spheres", [], []), ("set_boxes", [], [])], UPLOADS_AT_SETUP["r2"][1]),
    "so2": UPLOADS_AT_SETUP["so2"],
    "so3": ([("set_spheres", [], [])], UPLOADS_AT_SETUP["so3"][1]),
}
_CALLABLE = "the GPU path cannot call a Python function per interpolated state; "
WRONG_CHECKER_AT_SETUP = {
    "r2": _CALLABLE + "describe the obstacles with oxmpl_amd.base.SphereBoxValidityChecker",
    "so2": _CALLABLE + "describe the forbidden arcs with oxmpl_amd.base.SO2ArcValidityChecker",
    "so3": _CALLABLE + "describe the forbidden cones with oxmpl_amd.base.SO3ConeValidityChecker",
    "se3": _CALLABLE + "describe the body and the obstacles with oxmpl_amd.base.SE3RigidBodyValidityChecker",
}
WRONG_CHECKER_AT_REVALIDATE = {
    ("RRT", "r2"): "describe the obstacles with oxmpl_amd.base.SphereBoxValidityChecker",
    ("RRT", "so2"): "an SO(2) tree is re-checked against an SO2ArcValidityChecker",
    ("RRT", "so3"): "an SO(3) tree is re-checked against an SO3ConeValidityChecker",
    ("PRM", "r2"): "describe the obstacles with oxmpl_amd.base.SphereBoxValidityChecker",
    ("PRM", "so3"): "an SO(3) roadmap is re-checked against an SO3ConeValidityChecker",
}

# ---- the planners: constructor of the class surface, and what it passes to the handle's constructor
PLANNERS = {
    "RRT": lambda pd: RRT(0.5, 0.0625, pd, max_nodes=777, seed=3, problem_id=5, device=1, goal_sampler=capi.GOAL_SAMPLE_CENTRE),
    "RRTConnect": lambda pd: RRTConnect(0.5, 0.0625, pd, max_nodes=777, seed=3, problem_id=5, device=1),
    "RRTStar": lambda pd: RRTStar(0.5, 0.0625, 1.25, pd, max_nodes=777, seed=3, problem_id=5, device=1),
    "PRM": lambda pd: PRM(2.5, 0.75, pd, max_milestones=99, max_samples=1000, seed=3, stream=4, device=1),
}
PLANNER_ID = {"RRT": 0, "RRTConnect": 1, "RRTStar": 2}     # capi.PLANNER_*
BUILT_FOR = {"so2": ("RRT",), "so3": ("RRT", "PRM"), "se3": ("RRTConnect",)}   # (r2: every planner)
REFUSAL = {"so2": "SO(2) is built for RRT only", "so3": "SO(3) is built for RRT only", "se3": "SE(3) is built for RRTConnect only"}


def handle_of(planner):
    return "_prm" if isinstance(planner, PRM) else "_batch"


def constructor_record(planner, space):
    if planner == "PRM":
        return ("PRMRoadmap", dict(dim=DIM[space], bounds=BOUNDS[space], connection_radius=0.75, max_milestones=99, timeout=2.5,
                                   lvs_fraction=0.05, max_samples=1000, seed=3, stream=4, device=1, knn_k=0, space=KIND[space]))
    # search_radius reaches the library for every planner and means something to RRT* only: 0.0 and an omitted one are the same
    return ("RRTBatch", dict(dim=DIM[space], bounds=BOUNDS[space], max_distance=0.5, goal_bias=0.0625, n_problems=1, max_nodes=777,
                             lvs_fraction=0.05, stop_at_goal=True, seed=3, first_problem_id=5, device=1, kernel=0,
                             planner=PLANNER_ID[planner], search_radius=1.25 if planner == "RRTStar" else 0.0, space=KIND[space],
                             goal_sampler=0, debug_flags=0, star_pool_share=0, frozen_split=0))


def set_up(rec, planner, space, full=True):
    p = PLANNERS[planner](problem(space))
    p.setup(CHECKERS[space][int(full)])
    del rec.log[:]
    return p


# ================================================================ 1. every setup combination

@pytest.mark.parametrize("planner,space,checker", [(p, s, c) for p in PLANNERS for s in SPACES
                                                   for c in ["own, empty", "own, full"] + [o for o in SPACES if o != s] + ["lambda"]])
def test_setup_combination(rec, planner, space, checker):
    p = PLANNERS[planner](problem(space))
    attr = handle_of(p)
    previous = planted(rec, "PRMRoadmap" if planner == "PRM" else "RRTBatch")
    setattr(p, attr, previous)
    own = checker.startswith("own")
    full = checker == "own, full"
    c = CHECKERS[space][int(full)] if own else (lambda state: True) if checker == "lambda" else CHECKERS[checker][1]
    if planner == "PRM" and space == "se3":
        # refused; the text (and the way a SphereBoxValidityChecker fails) is left open, see the module's docstring
        with pytest.raises((TypeError, AttributeError)):
            p.setup(c)
        assert not [r for r in rec.log if r[0] == "PRMRoadmap"]
        return
    refused = None
    if space != "r2" and planner not in BUILT_FOR[space]:
        refused = REFUSAL[space]                       # the planner refusal comes first, whatever the checker is
    elif not own:
        refused = WRONG_CHECKER_AT_SETUP[space]
    if refused is not None:
        with pytest.raises(TypeError) as e:
            p.setup(c)
        assert str(e.value) == refused
        assert rec.log == [] and getattr(p, attr) is previous     # nothing closed, nothing created: the old handle is usable
        return
    p.setup(c)
    assert rec.log == [("close",), constructor_record(planner, space)] + UPLOADS_AT_SETUP[space][int(full)] + [SETUP_CALL[space]]
    assert type(getattr(p, attr)).__name__ == ("PRMRoadmap" if planner == "PRM" else "RRTBatch") and getattr(p, attr) is not previous


def test_setup_without_a_previous_handle_closes_nothing(rec):
    p = PLANNERS["RRT"](problem("r2"))
    p.setup(CHECKERS["r2"][0])
    assert rec.log == [constructor_record("RRT", "r2"), SETUP_CALL["r2"]]
    q = PLANNERS["PRM"](problem("so3"))
    del rec.log[:]
    q.setup(CHECKERS["so3"][0])
    assert rec.log == [constructor_record("PRM", "so3"), SETUP_CALL["so3"]]


def test_planner_constructors_refuse_what_is_no_problem_definition():
    for make in (lambda: RRT(0.5, 0.05, None), lambda: RRTStar(0.5, 0.05, 1.0, "pd"), lambda: PRM(1.0, 0.5, 3)):
        with pytest.raises(TypeError) as e:
            make()
        assert str(e.value) == "problem_definition must be a ProblemDefinition"


# ================================================================ 2. what comes back, per space

def assert_states(states, space, rows):
    assert [type(s) for s in states] == [STATE[space]] * len(rows)
    assert [s.values for s in states] == rows      # SO(2): 4.0 stays 4.0, a tree's states are not normalised again


RRT_FOR = {"r2": "RRT", "so2": "RRT", "so3": "RRT", "se3": "RRTConnect"}


@pytest.mark.parametrize("space", SPACES)
def test_rrt_solve_and_simplify_build_the_space_s_states(rec, space):
    p = set_up(rec, RRT_FOR[space], space)
    rows = np.array(ROWS[space])
    rec.canned.update(solve=np.array([capi.OK], dtype=np.int32), path=rows,
                      counts=dict(goal_node=np.array([2], dtype=np.int32), nodes=np.array([3], dtype=np.uint32)),
                      simplified_paths=(np.array([0, 2], dtype=np.uint64), rows[[0, 2]], np.array([0, 2], dtype=np.uint32),
                                        np.zeros(1), np.zeros(1), np.zeros(1, dtype=np.uint64)))
    path = p.solve(5.0)
    assert isinstance(path, Path) and rec.log == [("solve", 1 << 40, dict(timeout_s=5.0)), ("path", 0)]
    assert_states(path.states, space, ROWS[space])
    del rec.log[:]
    if space == "se3":
        with pytest.raises(TypeError) as e:
            p.simplify_solution()
        assert str(e.value) == "simplify_solution is not built for SE(3)" and rec.log == []
        return
    short = p.simplify_solution(max_span=4)
    assert rec.log == [("counts",), ("simplify_paths", 4), ("simplified_paths",)]
    assert isinstance(short, Path)
    assert_states(short.states, space, [ROWS[space][0], ROWS[space][2]])


def test_rrt_solve_statuses_and_arguments(rec):
    p = set_up(rec, "RRT", "r2")
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError) as e:
            p.solve(bad)
        assert str(e.value) == "timeout_secs must be a non-negative number"
    with pytest.raises(Exception) as e:
        p.solve(0)
    assert type(e.value) is Exception and str(e.value) == "No solution found within timeout." and rec.log == []
    for status, text in ((capi.ERR_TIMEOUT, "No solution found within timeout."), (capi.ERR_NO_SOLUTION_FOUND, "No solution found."),
                         (capi.ERR_INVALID_START_STATE, "Start state is not valid in the current StateSpace.")):
        rec.canned["solve"] = np.array([status], dtype=np.int32)
        with pytest.raises(Exception) as e:
            p.solve(1.0)
        assert type(e.value) is Exception and str(e.value) == text
    rec.canned["counts"] = dict(goal_node=np.array([-1], dtype=np.int32))
    with pytest.raises(Exception) as e:
        p.simplify_solution()
    assert type(e.value) is Exception and str(e.value) == "No solution found."


@pytest.mark.parametrize("space", ["r2", "so3"])
def test_prm_outputs_build_the_space_s_states(rec, space):
    p = set_up(rec, "PRM", space)
    rows = np.array(ROWS[space])
    offsets, nbrs = np.array([0, 1, 3, 4], dtype=np.uint64), np.array([1, 0, 2, 1], dtype=np.uint32)
    rec.canned.update(solve=(capi.OK, rows), roadmap=(rows, offsets, nbrs),
                      solve_batch=np.array([capi.OK, capi.ERR_INVALID_START_STATE, capi.OK], dtype=np.int32),
                      solve_batch_shortest=np.array([capi.ERR_NO_SOLUTION_FOUND, capi.OK, capi.ERR_TIMEOUT], dtype=np.int32),
                      batch_paths=(np.array([0, 2, 2, 3], dtype=np.uint64), np.array([0, 1, 2], dtype=np.uint32), rows))
    path = p.solve(1.5)
    assert isinstance(path, Path) and rec.log == [("solve", 1.5)]
    assert_states(path.states, space, ROWS[space])
    rec.canned["solve"] = (capi.ERR_NO_SOLUTION_FOUND, np.zeros((0, DIM[space])))
    with pytest.raises(Exception) as e:
        p.solve(1.5)
    assert type(e.value) is Exception and str(e.value) == "No solution found."

    pds = [problem(space)] * 3
    start, target, radius = SETUP_CALL[space][1:]
    del rec.log[:]
    out = p.solve_batch(pds, 2.0)
    assert rec.log == [("solve_batch", [start] * 3, [target] * 3, [radius] * 3, 2.0), ("batch_paths",)]
    assert isinstance(out[0], Path) and isinstance(out[2], Path)
    assert_states(out[0].states, space, ROWS[space][:2])
    assert_states(out[2].states, space, ROWS[space][2:])
    assert type(out[1]) is Exception and str(out[1]) == "Start state is not valid in the current StateSpace."   # returned, not raised
    del rec.log[:]
    out = p.solve_batch(pds, 2.0, shortest=True)
    assert rec.log == [("solve_batch_shortest", [start] * 3, [target] * 3, [radius] * 3, 2.0), ("batch_paths",)]
    assert [type(o) for o in out] == [Exception, Path, Exception]
    assert [str(out[0]), str(out[2])] == ["No solution found.", "No solution found within timeout."]
    assert out[1].states == []

    del rec.log[:]
    states, off, nb = p.get_roadmap()
    assert rec.log == [("roadmap",)] and off is offsets and nb is nbrs
    if space == "r2":
        assert states is rows                      # a real-vector roadmap's states stay the array the library filled
    else:
        assert_states(states, space, ROWS[space])


def test_prm_solve_batch_refuses_foreign_problems_before_any_call(rec):
    p = set_up(rec, "PRM", "r2")
    with pytest.raises(TypeError) as e:
        p.solve_batch([problem("r2"), "pd"], 1.0)
    assert str(e.value) == "problem_definitions must hold ProblemDefinition objects"
    other = ProblemDefinition.from_real_vector(RealVectorStateSpace(3, [(0.0, 1.0)] * 3), RealVectorState([0.5] * 3),
                                               Goal(RealVectorState([0.5] * 3), 0.1))
    for foreign in (problem("so3"), other):
        with pytest.raises(ValueError) as e:
            p.solve_batch([foreign], 1.0)
        assert str(e.value) == "every problem of a batch must share the planner's state space"
    assert rec.log == []


def test_prm_set_problem_definition_and_plain_forwards(rec):
    p = PLANNERS["PRM"](problem("r2"))
    p.set_problem_definition(problem("so2"))       # as permissive as ever: no handle, nothing to tell
    assert rec.log == [] and p.num_milestones == 0
    with pytest.raises(TypeError) as e:
        p.set_problem_definition(None)
    assert str(e.value) == "problem_definition must be a ProblemDefinition"
    p = set_up(rec, "PRM", "r2")
    rec.canned.update(sizes=(7, 12, 40), grow=(1, 2), components="c", prune="p")
    p.set_problem_definition(problem("r2"))
    p.construct_roadmap()
    assert p.num_milestones == 7
    assert p.grow_roadmap(5, max_samples=9) == (1, 2) and p.grow_roadmap(5, new_stream=8) == (1, 2)
    assert p.components() == "c" and p.prune_roadmap(invalid=1, keep=[1, 0], min_size=2, largest=0) == "p"
    p.set_roadmap([RealVectorState([1.0, 0.0]), [2.0, 0.5]], [0, 1, 2], [1, 0])
    assert rec.log == [("set_problem",) + SETUP_CALL["r2"][1:], ("construct_roadmap",), ("sizes",), ("grow", 5, 9, None),
                       ("grow", 5, 0, 8), ("components",), ("prune", True, [1, 0], 2, False),
                       ("set_roadmap", [[1.0, 0.0], [2.0, 0.5]], [0, 1, 2], [1, 0])]


# ================================================================ 3. revalidate

@pytest.mark.parametrize("planner,space", sorted(WRONG_CHECKER_AT_REVALIDATE))
def test_revalidate_uploads(rec, planner, space):
    p = set_up(rec, planner, space)
    if planner == "RRT":
        call, want = ("revalidate_trees",), 2
        rec.canned["revalidate_trees"] = dict(n_removed=np.array([2], dtype=np.uint32), goal_lost=np.array([False]))
    else:
        call, want = ("revalidate",), ("mask", 3)
        rec.canned["revalidate"] = want
    assert p.revalidate() == want and rec.log == [call]         # no checker: no upload
    for full in (0, 1):
        del rec.log[:]
        assert p.revalidate(CHECKERS[space][full]) == want
        assert rec.log == UPLOADS_AT_REVALIDATE[space][full] + [call]
        if planner == "RRT":
            assert p._checker is CHECKERS[space][full]
    for other in [s for s in SPACES if s != space] + ["lambda"]:
        del rec.log[:]
        with pytest.raises(TypeError) as e:
            p.revalidate((lambda state: True) if other == "lambda" else CHECKERS[other][1])
        assert str(e.value) == WRONG_CHECKER_AT_REVALIDATE[planner, space] and rec.log == []


@pytest.mark.parametrize("planner", ["RRTConnect", "RRTStar"])
def test_revalidate_is_refused_for_the_other_tree_planners(rec, planner):
    for p in (PLANNERS[planner](problem("r2")), set_up(rec, planner, "r2")):      # refused before "not set up", too
        with pytest.raises(TypeError) as e:
            p.revalidate()
        assert str(e.value) == "revalidate is built for RRT only (not RRTConnect, not RRTStar)" and rec.log == []


# ================================================================ 4. error translation

STATUSES = [capi.ERR_TIMEOUT, capi.ERR_NO_SOLUTION_FOUND, capi.ERR_PLANNER_UNINITIALISED, capi.ERR_INVALID_START_STATE,
            capi.ERR_UNSAMPLED_STATE_SPACE, capi.ERR_BAD_ARG, capi.ERR_UNBOUNDED, capi.ERR_ZERO_VOLUME, capi.ERR_CAPACITY, capi.ERR_HIP]
MESSAGES = {1: "No solution found within timeout.", 2: "No solution found.", 3: UNINITIALISED,
            4: "Start state is not valid in the current StateSpace.", 5: "StateSpace is not sampled. Either Tree or Roadmap is empty."}
AT_CREATE = {capi.ERR_UNBOUNDED, capi.ERR_ZERO_VOLUME, capi.ERR_BAD_ARG}
AT_REFUSED_ARGUMENT = {capi.ERR_BAD_ARG, capi.ERR_CAPACITY}
# (planner, space, the handle method that fails, the public call, statuses that become ValueError, reference messages?)
SITES = {
    "RRT.setup r2": ("RRT", "r2", "__init__", None, AT_CREATE, False),
    "RRTStar.setup r2": ("RRTStar", "r2", "__init__", None, AT_CREATE, False),
    "RRT.setup so2": ("RRT", "so2", "__init__", None, AT_CREATE, False),
    "RRT.setup so3": ("RRT", "so3", "__init__", None, AT_CREATE, False),
    "RRTConnect.setup se3": ("RRTConnect", "se3", "__init__", None, AT_CREATE, False),
    "PRM.setup r2": ("PRM", "r2", "__init__", None, AT_CREATE, False),
    "PRM.setup so3": ("PRM", "so3", "__init__", None, AT_CREATE, False),
    "RRT.revalidate": ("RRT", "r2", "revalidate_trees", lambda p: p.revalidate(), set(), True),
    "PRM.solve_batch": ("PRM", "r2", "solve_batch", lambda p: p.solve_batch([problem("r2")], 1.0), set(), True),
    "PRM.solve_batch shortest": ("PRM", "so3", "solve_batch_shortest", lambda p: p.solve_batch([problem("so3")], 1.0, shortest=True),
                                 set(), True),
    "PRM.set_roadmap": ("PRM", "r2", "set_roadmap", lambda p: p.set_roadmap([[1.0, 0.0]], [0, 0], []), AT_REFUSED_ARGUMENT, False),
    "PRM.revalidate": ("PRM", "r2", "revalidate", lambda p: p.revalidate(), set(), True),
    "PRM.revalidate so3, new checker": ("PRM", "so3", "revalidate", lambda p: p.revalidate(CHECKERS["so3"][1]), set(), True),
    "PRM.grow_roadmap": ("PRM", "r2", "grow", lambda p: p.grow_roadmap(4), AT_REFUSED_ARGUMENT, True),
    "PRM.components": ("PRM", "r2", "components", lambda p: p.components(), set(), True),
    "PRM.prune_roadmap": ("PRM", "r2", "prune", lambda p: p.prune_roadmap(largest=True), AT_REFUSED_ARGUMENT, True),
}


def _left_open(site, status):
    """the library never gives ERR_UNBOUNDED for an SO(2) / SO(3) config: see the module's docstring"""
    return SITES[site][2] == "__init__" and SITES[site][1] in ("so2", "so3") and status == capi.ERR_UNBOUNDED


@pytest.mark.parametrize("site,status", [(s, st) for s in SITES for st in STATUSES if not _left_open(s, st)])
def test_error_translation(rec, site, status):
    planner, space, method, call, value_errors, messages = SITES[site]
    if call is None:
        p = PLANNERS[planner](problem(space))
        call = lambda p: p.setup(CHECKERS[space][1])
    else:
        p = set_up(rec, planner, space)
    rec.fail[method] = status
    with pytest.raises(Exception) as e:
        call(p)
    if status in value_errors:
        assert type(e.value) is ValueError and str(e.value) == str(capi.OxhipError(status, "x"))
    elif messages and status in MESSAGES:
        assert type(e.value) is Exception and str(e.value) == MESSAGES[status]
    else:
        assert type(e.value) is capi.OxhipError and e.value.status == status     # the library's own error, untouched
    if method == "__init__":
        assert getattr(p, handle_of(p)) is None


def test_the_messages_are_the_reference_s():
    assert geometric._MESSAGES == MESSAGES


# ================================================================ 5. planners that were never set up

def test_methods_of_a_planner_that_was_never_set_up(rec, tmp_path):
    r = PLANNERS["RRT"](problem("r2"))
    p = PLANNERS["PRM"](problem("r2"))
    calls = [lambda: r.solve(1.0), lambda: r.simplify_solution(), lambda: r.revalidate(), lambda: r.revalidate(CHECKERS["r2"][1]),
             lambda: p.construct_roadmap(), lambda: p.solve(1.0), lambda: p.solve_batch([problem("r2")], 1.0),
             lambda: p.set_roadmap([], [0], []), lambda: p.revalidate(), lambda: p.revalidate(CHECKERS["r2"][1]),
             lambda: p.grow_roadmap(1), lambda: p.components(), lambda: p.prune_roadmap(largest=True),
             lambda: p.save_roadmap(str(tmp_path / "never.npz"))]
    for call in calls:
        with pytest.raises(Exception) as e:
            call()
        assert type(e.value) is Exception and str(e.value) == UNINITIALISED
    assert rec.log == [] and not (tmp_path / "never.npz").exists()


# ================================================================ 6. a roadmap in a file

@pytest.mark.parametrize("space,name", [("r2", "real_vector"), ("so3", "so3")])
def test_roadmap_file_round_trip(rec, tmp_path, space, name):
    p = set_up(rec, "PRM", space)
    rows = np.array(ROWS[space])
    offsets, nbrs = np.array([0, 1, 3, 4], dtype=np.uint64), np.array([1, 0, 2, 1], dtype=np.uint32)
    rec.canned["roadmap"] = (rows, offsets, nbrs)
    f = str(tmp_path / "roadmap.npz")
    p.save_roadmap(f)
    with np.load(f, allow_pickle=False) as z:
        assert sorted(z.files) == ["dim", "neighbours", "offsets", "space", "states"]
        assert str(z["space"]) == name and int(z["dim"]) == DIM[space] and z["dim"].dtype == np.uint32
        assert z["states"].tolist() == ROWS[space]
    q = set_up(rec, "PRM", space)
    q.load_roadmap(f)
    assert rec.log == [("set_roadmap", ROWS[space], [0, 1, 3, 4], [1, 0, 2, 1])]

    # a file of another space, or of another width, is refused before any call
    other = "so3" if space == "r2" else "r2"
    del rec.log[:]
    with pytest.raises(ValueError) as e:
        set_up(rec, "PRM", other).load_roadmap(f)
    assert str(e.value) == ("roadmap file is for %s dim %d, the planner's space is %s dim %d"
                            % (name, DIM[space], "so3" if space == "r2" else "real_vector", DIM[other]))
    assert rec.log == []
    g = str(tmp_path / "malformed.npz")
    with open(g, "wb") as fh:
        np.savez(fh, states=rows[:, :1], offsets=offsets, neighbours=nbrs, space=np.array(name), dim=np.array(DIM[space], dtype=np.uint32))
    with pytest.raises(ValueError) as e:
        q.load_roadmap(g)
    assert str(e.value) == "roadmap file is malformed: states (3, 1), offsets (4,)"
    with open(g, "wb") as fh:
        np.savez(fh, states=rows, offsets=offsets[:3], neighbours=nbrs, space=np.array(name), dim=np.array(DIM[space], dtype=np.uint32))
    with pytest.raises(ValueError) as e:
        q.load_roadmap(g)
    assert str(e.value) == "roadmap file is malformed: states (3, %d), offsets (3,)" % DIM[space]
    assert rec.log == []
