"""Mirror of `oxmpl_py.base` (reference: oxmpl-py/src/base/*.rs) for the GPU RRT path.

Same class names, constructor signatures and error types as the reference's PyO3 classes
(`RealVectorState`, `RealVectorStateSpace`, `ProblemDefinition.from_real_vector`, `Path`), so the
reference's Python test (oxmpl-py/tests/test_rrt_rvss.py) ports by changing the import line and
replacing its per-state Python callback by a descriptor object: a Python callable evaluated once
per interpolated state under the GIL (oxmpl-py/src/base/state_validity_checker.rs:30-48) is the
opposite of a batched device path, and there is deliberately no CPU fallback that would run it.

Everything that computes (`distance`, validity) is evaluated by the HIP library.
"""
import math

import numpy as np

from . import capi


class RealVectorState:
    """oxmpl_py.base.RealVectorState (oxmpl-py/src/base/real_vector_state.rs:17-40)"""

    def __init__(self, values):
        self._values = [float(v) for v in values]

    @property
    def values(self):
        return list(self._values)

    def __repr__(self):
        return "<RealVectorState values=%r>" % (self._values,)


def _device_distance(op, state1, state2):
    """`op` of the two states as one-row arrays, on the device -> the one result"""
    return float(op(np.array([state1.values], dtype=np.float64), np.array([state2.values], dtype=np.float64))[0])


class _StateSpace:
    """What the four state spaces share.  Each sets `dimension` (the width of a state's `values`) and
    `longest_valid_segment_fraction` (0.05, as the reference) in its constructor."""

    def set_longest_valid_segment_fraction(self, fraction):
        if 0.0 < fraction <= 1.0:
            self.longest_valid_segment_fraction = float(fraction)
        elif fraction <= 0.0:
            self.longest_valid_segment_fraction = 0.0
        else:
            self.longest_valid_segment_fraction = 1.0


class RealVectorStateSpace(_StateSpace):
    """oxmpl_py.base.RealVectorStateSpace (oxmpl-py/src/base/real_vector_state_space.rs:15-57).
    Construction errors are ValueError with the reference's messages (error.rs:40-52)."""

    def __init__(self, dimension, bounds=None):
        dimension = int(dimension)
        if bounds is not None:
            bounds = [(float(lo), float(hi)) for lo, hi in bounds]
            if len(bounds) != dimension:
                raise ValueError("provided bounds length (%d) does not match specified dimension (%d)."
                                 % (len(bounds), dimension))
            for lo, hi in bounds:
                if lo >= hi:
                    raise ValueError("Lower bound %s is greater than upper bound %s." % (lo, hi))
        else:
            if dimension == 0:
                raise ValueError("Cannot create 0-dimensional unbounded space.")
            bounds = [(-math.inf, math.inf)] * dimension
        self.dimension = dimension
        self.bounds = bounds
        self.longest_valid_segment_fraction = 0.05

    def distance(self, state1, state2):
        return _device_distance(capi.distance_batch, state1, state2)

    def get_maximum_extent(self):
        if any((not math.isfinite(lo)) or (not math.isfinite(hi)) for lo, hi in self.bounds):
            return 1.0
        # sqrt of the sequential sum of squared widths (real_vector_state_space.rs:103-118), on the device
        z = np.zeros((1, self.dimension))
        w = np.array([[hi - lo for lo, hi in self.bounds]], dtype=np.float64)
        return float(capi.distance_batch(w, z)[0])


class SphereBoxValidityChecker:
    """Device-describable StateValidityChecker: a state is valid iff it lies strictly outside every
    sphere (distance(centre, p) > radius, the README's predicate) and inside no box (faces
    inclusive, the wall of the reference's tests).  Pass it to RRT.setup() where the reference takes
    a Python callable."""

    def __init__(self, spheres=(), boxes=()):
        self.spheres = [([float(v) for v in c], float(r)) for c, r in spheres]
        self.boxes = [([float(v) for v in lo], [float(v) for v in hi]) for lo, hi in boxes]


class SO3State:
    """oxmpl_py.base.SO3State (oxmpl-py/src/base/so3_state.rs): a rotation as the quaternion (x, y, z, w).  Not normalised
    on construction, as in the reference (oxmpl/src/base/states/so3_state.rs:21-30)."""

    def __init__(self, x, y, z, w):
        self.x, self.y, self.z, self.w = float(x), float(y), float(z), float(w)

    @staticmethod
    def identity():
        return SO3State(0.0, 0.0, 0.0, 1.0)

    @property
    def values(self):
        return [self.x, self.y, self.z, self.w]

    def __eq__(self, other):
        return isinstance(other, SO3State) and self.values == other.values

    def __repr__(self):
        return "<SO3State x=%r, y=%r, z=%r, w=%r>" % (self.x, self.y, self.z, self.w)


class SO3StateSpace(_StateSpace):
    """oxmpl_py.base.SO3StateSpace (oxmpl-py/src/base/so3_state_space.rs): SO3StateSpace(bounds=None | (SO3State, max_angle)).
    None: the identity and PI, every rotation.  A negative max_angle is ValueError (StateSpaceError::InvalidAngularDistance);
    max_angle is clamped to PI (oxmpl/src/base/spaces/so3_state_space.rs:57-76).  `distance` is evaluated by the HIP library."""

    def __init__(self, bounds=None):
        if bounds is None:
            centre, max_angle = SO3State.identity(), math.pi
        else:
            centre, max_angle = bounds
            if not isinstance(centre, SO3State):
                raise TypeError("bounds must be (SO3State, max_angle)")
            max_angle = float(max_angle)
            if max_angle < 0.0:
                raise ValueError("Invalid angular distance: %s must not be negative." % max_angle)
            max_angle = math.pi if max_angle != max_angle else min(max_angle, math.pi)
        self.bounds = (centre, max_angle)
        self.dimension = 4
        self.longest_valid_segment_fraction = 0.05

    def distance(self, state1, state2):
        return _device_distance(lambda a, b: capi.so3_op_batch(0, a, b), state1, state2)

    def get_maximum_extent(self):
        return 0.5 * math.pi

    def config_bounds(self):
        """the C ABI's reading of oxhip_rrt_config.bounds for SO(3): (cx, cy, cz, cw, max_angle)"""
        return self.bounds[0].values + [self.bounds[1]]


class SO3ConeValidityChecker:
    """Device-describable StateValidityChecker of SO(3): a state is valid iff distance(centre, q) > radius for every cone
    (strict) -- the ForbiddenConeChecker of oxmpl/tests/rrt_so3ss_tests.rs:46-56, one or more of them.  Pass it to
    RRT.setup() with an SO(3) ProblemDefinition."""

    def __init__(self, cones=()):
        self.cones = []
        for centre, radius in cones:
            c = centre.values if isinstance(centre, SO3State) else [float(v) for v in centre]
            if len(c) != 4:
                raise ValueError("a cone's centre is a quaternion (x, y, z, w)")
            self.cones.append((list(c), float(radius)))


def _so2_normalise(v):
    # (v + PI).rem_euclid(2 PI) - PI: math.fmod is C's fmod, exact, as Rust's `%` on f64
    r = math.fmod(v + math.pi, 2.0 * math.pi)
    if r < 0.0:
        r = r + 2.0 * math.pi
    return r - math.pi


class SO2State:
    """oxmpl_py.base.SO2State: an angle in radians.  SO2State(value) normalises to [-PI, PI) as SO2State::new does
    (oxmpl/src/base/states/so2_state.rs:33-37)."""

    def __init__(self, value):
        self.value = _so2_normalise(float(value))

    @property
    def values(self):
        return [self.value]

    def __eq__(self, other):
        return isinstance(other, SO2State) and self.value == other.value

    def __repr__(self):
        return "<SO2State value=%r>" % self.value


class SO2StateSpace(_StateSpace):
    """oxmpl_py.base.SO2StateSpace: SO2StateSpace(bounds=None | (lo, hi)).  None: the full circle (-PI, PI).  lo >= hi is
    ValueError (StateSpaceError::InvalidBound); the bounds are clamped to [-PI, PI]
    (oxmpl/src/base/spaces/so2_state_space.rs:57-74).  `distance` is add, subtract and fmod only: evaluated here, the bits
    are the device's."""

    def __init__(self, bounds=None):
        lo, hi = (-math.pi, math.pi) if bounds is None else (float(bounds[0]), float(bounds[1]))
        if not lo < hi:
            raise ValueError("Invalid bound: lower %s must be less than upper %s." % (lo, hi))
        self.bounds = (max(lo, -math.pi), min(hi, math.pi))
        self.dimension = 1
        self.longest_valid_segment_fraction = 0.05

    def distance(self, state1, state2):
        return abs(_so2_normalise(state1.value - state2.value))

    def get_maximum_extent(self):
        return math.pi

    def config_bounds(self):
        """the C ABI's reading of oxhip_rrt_config.bounds for SO(2): (lo, hi)"""
        return [self.bounds[0], self.bounds[1]]


class SO2ArcValidityChecker:
    """Device-describable StateValidityChecker of SO(2): a state is valid iff its normalised value lies in no arc
    [min, max], closed on both ends -- the ForbiddenAngleChecker of oxmpl/tests/rrt_so2ss_tests.rs, any number of them.
    Pass it to RRT.setup() with an SO(2) ProblemDefinition."""

    def __init__(self, arcs=()):
        self.arcs = [(float(lo), float(hi)) for lo, hi in arcs]


class SE3State:
    """A rigid-body pose: position (x, y, z) and a rotation (SO3State).  The reference has no SE(3) state yet
    (docs/BACKLOG.md:12-14); this is the compound of its RealVectorState and SO3State.  `values` is the C ABI's row
    (x, y, z, qx, qy, qz, qw)."""

    def __init__(self, x, y, z, rotation):
        if not isinstance(rotation, SO3State):
            raise TypeError("rotation must be an SO3State")
        self.x, self.y, self.z, self.rotation = float(x), float(y), float(z), rotation

    @staticmethod
    def from_values(row):
        row = [float(v) for v in row]
        if len(row) != 7:
            raise ValueError("an SE(3) row is (x, y, z, qx, qy, qz, qw)")
        return SE3State(row[0], row[1], row[2], SO3State(*row[3:]))

    @property
    def values(self):
        return [self.x, self.y, self.z] + self.rotation.values

    def __eq__(self, other):
        return isinstance(other, SE3State) and self.values == other.values

    def __repr__(self):
        return "<SE3State x=%r, y=%r, z=%r, rotation=%r>" % (self.x, self.y, self.z, self.rotation)


class SE3StateSpace(_StateSpace):
    """SE(3) = R^3 x SO(3), assembled from the reference's RealVectorStateSpace(3) and SO3StateSpace with OMPL's weights
    (include/oxmpl_hip.h, OXHIP_SPACE_SE3): SE3StateSpace(bounds_xyz, rotation_bounds=None | (SO3State, max_angle)).
    distance = distance_R3 + distance_SO3, evaluated by the HIP library; extent = extent_R3 + 0.5 * PI."""

    def __init__(self, bounds_xyz, rotation_bounds=None):
        self.position = RealVectorStateSpace(3, bounds_xyz)
        self.rotation = SO3StateSpace(rotation_bounds)
        self.dimension = 7
        self.longest_valid_segment_fraction = 0.05

    def distance(self, state1, state2):
        return _device_distance(lambda a, b: capi.se3_op_batch(0, a, b), state1, state2)

    def get_maximum_extent(self):
        return self.position.get_maximum_extent() + 0.5 * math.pi

    def config_bounds(self):
        """the C ABI's reading of oxhip_rrt_config.bounds for SE(3): the (lo, hi) pairs of x, y, z, then (cx, cy, cz, cw, max_angle)"""
        return [v for pair in self.position.bounds for v in pair] + self.rotation.config_bounds()


class SE3RigidBodyValidityChecker:
    """Device-describable StateValidityChecker of SE(3): a rigid body of spheres (centre in the body frame, radius; 1 .. 16 of
    them, default a point at the origin) among world spheres.  A state is valid iff every body sphere, carried to
    rot(q, centre) + (x, y, z), lies strictly outside every obstacle: distance > r_body + r_obstacle.  Pass it to
    RRTConnect.setup() with an SE(3) ProblemDefinition."""

    def __init__(self, body=None, obstacles=()):
        body = [([0.0, 0.0, 0.0], 0.0)] if body is None else list(body)
        if not 1 <= len(body) <= capi.SE3_MAX_BODY:
            raise ValueError("a body has 1 .. %d spheres" % capi.SE3_MAX_BODY)
        self.body, self.obstacles = [], []
        for name, src, dst in (("body", body, self.body), ("obstacle", obstacles, self.obstacles)):
            for centre, radius in src:
                c = [float(v) for v in centre]
                if len(c) != 3:
                    raise ValueError("a %s sphere's centre is (x, y, z)" % name)
                dst.append((c, float(radius)))
        if any(not (r >= 0.0 and math.isfinite(r)) for _, r in self.body):
            raise ValueError("a body sphere's radius must be finite and >= 0")


class ProblemDefinition:
    """oxmpl_py.base.ProblemDefinition (oxmpl-py/src/base/problem_definition.rs:43-75)"""

    def __init__(self, space, start_state, goal):
        self.space, self.start_state, self.goal = space, start_state, goal

    @staticmethod
    def _from(space_cls, state_cls, space, start_state, goal):
        """the body of the four from_* constructors: a space_cls, a ball goal and two state_cls states -> ProblemDefinition"""
        if not isinstance(space, space_cls):   # ("an SO3StateSpace", "a RealVectorStateSpace")
            raise TypeError("space must be %s %s" % ("an" if space_cls.__name__.startswith("S") else "a", space_cls.__name__))
        if not hasattr(goal, "target") or not hasattr(goal, "radius"):
            raise TypeError("the GPU path needs a ball goal: an object with `target` and `radius` attributes")
        if state_cls is RealVectorState:       # as the reference: any state of the space's width
            if len(start_state.values) != space.dimension or len(goal.target.values) != space.dimension:
                raise ValueError("state dimension does not match the space")
        elif not isinstance(start_state, state_cls) or not isinstance(goal.target, state_cls):
            raise TypeError("start_state and goal.target must be %s" % state_cls.__name__)
        return ProblemDefinition(space, start_state, goal)

    @staticmethod
    def from_real_vector(space, start_state, goal):
        """`goal` is any object with a `target` (RealVectorState) and a `radius`: the reference's
        CircularGoal classes qualify as they are.  is_satisfied(s) = distance(s, target) <= radius;
        the device goal sampler returns `target` (README.md:160-162), `goal.sample_goal` is not called."""
        return ProblemDefinition._from(RealVectorStateSpace, RealVectorState, space, start_state, goal)

    @staticmethod
    def from_so3(space, start_state, goal):
        """oxmpl_py ProblemDefinition.from_so3 (oxmpl-py/src/base/problem_definition.rs:105-131).  `goal`: any object with a
        `target` (SO3State) and a `radius`; is_satisfied(s) = distance(s, target) <= radius, sample_goal() = target."""
        return ProblemDefinition._from(SO3StateSpace, SO3State, space, start_state, goal)

    @staticmethod
    def from_so2(space, start_state, goal):
        """oxmpl_py ProblemDefinition.from_so2.  `goal`: any object with a `target` (SO2State) and a `radius`;
        is_satisfied(s) = distance(s, target) <= radius, sample_goal() = target (the fixture's arc sampler is not built)."""
        return ProblemDefinition._from(SO2StateSpace, SO2State, space, start_state, goal)

    @staticmethod
    def from_se3(space, start_state, goal):
        """`goal`: any object with a `target` (SE3State) and a `radius`; is_satisfied(s) = distance(s, target) <= radius in the
        SE(3) distance, sample_goal() = target."""
        return ProblemDefinition._from(SE3StateSpace, SE3State, space, start_state, goal)


class Path:
    """oxmpl_py.base.Path (oxmpl-py/src/base/path.rs:27-99)"""

    def __init__(self, states):
        self._states = list(states)

    @staticmethod
    def from_real_vector_states(states):
        return Path(states)

    @property
    def states(self):
        return list(self._states)

    def __len__(self):
        return len(self._states)

    def __repr__(self):
        return "<Path with %d states>" % len(self._states)
