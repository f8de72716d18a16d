//! `oxmpl-hip`: oxmpl's planners on an AMD MI355X, behind oxmpl's own `Planner` trait.
//!
//! ```ignore
//! let checker = Arc::new(SphereField { spheres: vec![(vec![0.0, 0.0], 2.0)] });      // impl DeviceValidityChecker
//! let mut planner = HipRRT::new(0.5, 0.05, checker.clone());                         // RRT::new(0.5, 0.05)
//! planner.setup(problem_def, checker);                                               // Planner::setup
//! let path = planner.solve(Duration::from_secs(5))?;                                 // Planner::solve
//! ```
//!
//! # How the validity checker crosses the boundary
//!
//! `Planner::setup` (oxmpl/src/base/planner.rs:42-46) hands the planner an `Arc<dyn StateValidityChecker<S>>`.
//! That trait (oxmpl/src/base/validity.rs:39-48) has one method, `is_valid`, and no `Any` supertrait, so nothing
//! can be recovered from the trait object but verdicts on single states -- and a GPU cannot call back into Rust
//! per interpolated state.  The obstacle *description* therefore enters through the constructor, typed:
//! `HipRRT::new(max_distance, goal_bias, checker: Arc<D>)` with `D: DeviceValidityChecker`.  `setup` keeps its
//! trait signature; the `dyn` checker it receives is used for what it can do -- it is probed on the start
//! state and on a deterministic set of states inside the bounds, and `setup` panics if its verdicts differ from
//! the description's, so the two cannot silently drift apart.  There is no CPU fallback in this crate.
//!
//! The goal is not erased by the trait (`G` is a type parameter of `Planner`), so `G: DeviceGoal` is enough.
//!
//! Source only: the repository's build image has no Rust toolchain.

pub mod ffi;

use std::ffi::CStr;
use std::ptr;
use std::sync::Arc;
use std::time::Duration;

use oxmpl::base::error::PlanningError;
use oxmpl::base::goal::GoalSampleableRegion;
use oxmpl::base::planner::{Path, Planner};
use oxmpl::base::problem_definition::ProblemDefinition;
use oxmpl::base::space::{RealVectorStateSpace, SO2StateSpace, SO3StateSpace, StateSpace};
use oxmpl::base::state::{RealVectorState, SO3State};
use oxmpl::base::validity::StateValidityChecker;

type Pd<G> = ProblemDefinition<RealVectorState, RealVectorStateSpace, G>;

/// A `StateValidityChecker` that can describe itself to the device: a state is valid iff it lies strictly
/// outside every sphere (`distance(centre, p) > radius`, the predicate of README.md:147-150) and inside no
/// axis-aligned box (faces inclusive, the wall of oxmpl/tests/rrt_rvss_tests.rs:24-36).  `is_valid` of the
/// implementor must be exactly that predicate; `HipRRT::setup` spot-checks it.
pub trait DeviceValidityChecker: StateValidityChecker<RealVectorState> {
    /// `(centre, radius)` pairs
    fn spheres(&self) -> Vec<(Vec<f64>, f64)> {
        Vec::new()
    }
    /// `(lower corner, upper corner)` pairs
    fn boxes(&self) -> Vec<(Vec<f64>, Vec<f64>)> {
        Vec::new()
    }
}

/// A goal the device understands: `is_satisfied(s) = distance(s, centre) <= radius`.  The device samples the
/// region at its centre (no RNG draw), which is what README.md:160-162 does; goals that sample elsewhere plan
/// correctly but draw a different random stream than the CPU planner would.
pub trait DeviceGoal: GoalSampleableRegion<RealVectorState> {
    fn ball(&self) -> (Vec<f64>, f64);
    /// what `sample_goal` draws on the device (default: the centre, no random word -- README.md:160-162)
    fn sampling(&self) -> GoalSampling {
        GoalSampling::Centre
    }
}

/// What `sample_goal` draws on the device (`oxhip_goal_sampler`).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum GoalSampling {
    /// the ball's centre, no random word consumed (`README.md:160-162`)
    Centre,
    /// uniform in the disc, as the `CircularGoalRegion` of `oxmpl/tests/rrt_rvss_tests.rs:55-66` samples it:
    /// `random_range(0.0..2.0 * PI)`, then `random::<f64>().sqrt()`; 2-D spaces.  The device evaluates cos / sin with its own
    /// portable routine (within one ulp of libm): results are within 1e-6 relative of the CPU path, not bit-identical.
    UniformDisc,
}

/// Deterministic knobs the reference does not have (its only stop is the wall clock, rrt.rs:172-174, and its RNG
/// is OS-seeded, rrt.rs:167).
#[derive(Clone, Copy, Debug)]
pub struct HipOptions {
    /// tree capacity; a full tree ends `solve` with `NoSolutionFound`
    pub max_nodes: u32,
    /// ChaCha12 key (LE(seed) || 0^24) and stream id of this planner's random stream
    pub seed: u64,
    pub stream: u64,
    /// HIP device ordinal
    pub device: i32,
}

impl Default for HipOptions {
    fn default() -> Self {
        HipOptions { max_nodes: 10_000, seed: 0, stream: 0, device: 0 }
    }
}

fn last_error() -> String {
    unsafe { CStr::from_ptr(ffi::oxhip_last_error_string()).to_string_lossy().into_owned() }
}

fn to_planning_error(status: i32) -> PlanningError {
    match status {
        ffi::OXHIP_ERR_TIMEOUT => PlanningError::Timeout,
        ffi::OXHIP_ERR_PLANNER_UNINITIALISED => PlanningError::PlannerUninitialised,
        ffi::OXHIP_ERR_INVALID_START_STATE => PlanningError::InvalidStartState,
        ffi::OXHIP_ERR_UNSAMPLED_STATE_SPACE => PlanningError::UnsampledStateSpace,
        _ => PlanningError::NoSolutionFound,
    }
}

/// `longest_valid_segment_fraction` is a private field of `RealVectorStateSpace` (rvss.rs:25); its public trace is
/// `get_longest_valid_segment_length() = extent * fraction` (rvss.rs:251-253).  The C ABI takes the fraction and
/// repeats that product, so look for the double whose product with the extent reproduces the length bit for bit
/// (the quotient, or one of its neighbours).
fn fraction_of(space: &RealVectorStateSpace) -> f64 {
    let extent = space.get_maximum_extent();
    let length = space.get_longest_valid_segment_length();
    if !(extent > 0.0) {
        return 0.05;
    }
    let q = length / extent;
    for step in [0i64, 1, -1, 2, -2] {
        let cand = f64::from_bits((q.to_bits() as i64 + step) as u64);
        if extent * cand == length {
            return cand;
        }
    }
    q
}

fn flatten(rows: &[Vec<f64>], dim: usize, what: &str) -> Vec<f64> {
    let mut out = Vec::with_capacity(rows.len() * dim);
    for r in rows {
        assert_eq!(r.len(), dim, "{} has the wrong dimension", what);
        out.extend_from_slice(r);
    }
    out
}

/// the description's own verdict, on the host: used only to cross-check the `dyn` checker in `setup`
fn described_valid(spheres: &[(Vec<f64>, f64)], boxes: &[(Vec<f64>, Vec<f64>)], p: &[f64]) -> bool {
    for (c, r) in spheres {
        let mut acc = 0.0;
        for (a, b) in c.iter().zip(p) {
            acc += (a - b) * (a - b);
        }
        if !(acc.sqrt() > *r) {
            return false;
        }
    }
    for (lo, hi) in boxes {
        if lo.iter().zip(hi).zip(p).all(|((l, h), x)| l <= x && x <= h) {
            return false;
        }
    }
    true
}

/// which of the reference's tree planners a `HipRRT` stands for
#[derive(Clone, Copy, Debug, PartialEq)]
pub enum TreePlanner {
    /// `geometric::RRT` (rrt.rs)
    Rrt,
    /// `geometric::RRTConnect` (rrt_connect.rs)
    RrtConnect,
    /// `geometric::RRTStar` (rrt_star.rs) with its `search_radius`
    RrtStar { search_radius: f64 },
}

/// GPU twin of `oxmpl::geometric::RRT` (and, through `TreePlanner`, of `RRTConnect` / `RRTStar`): same public
/// parameters (rrt.rs:53-57), same trait, one planning problem per instance.  Batches of thousands of problems
/// skip the trait and drive `ffi::oxhip_rrt_batch_*` with `n_problems = P` (what bench.py does through ctypes).
pub struct HipRRT<D: DeviceValidityChecker, G: DeviceGoal> {
    pub max_distance: f64,
    pub goal_bias: f64,
    pub planner: TreePlanner,
    pub options: HipOptions,
    checker: Arc<D>,
    problem_def: Option<Arc<Pd<G>>>,
    batch: *mut ffi::OxhipRrtBatch,
}

impl<D: DeviceValidityChecker, G: DeviceGoal> HipRRT<D, G> {
    /// `RRT::new(max_distance, goal_bias)` (rrt.rs:75-83) plus the typed obstacle description (see the crate docs)
    pub fn new(max_distance: f64, goal_bias: f64, checker: Arc<D>) -> Self {
        HipRRT {
            max_distance,
            goal_bias,
            planner: TreePlanner::Rrt,
            options: HipOptions::default(),
            checker,
            problem_def: None,
            batch: ptr::null_mut(),
        }
    }

    /// `RRTStar::new(max_distance, goal_bias, search_radius)` (rrt_star.rs:65-77)
    pub fn new_star(max_distance: f64, goal_bias: f64, search_radius: f64, checker: Arc<D>) -> Self {
        let mut p = Self::new(max_distance, goal_bias, checker);
        p.planner = TreePlanner::RrtStar { search_radius };
        p
    }

    /// `RRTConnect::new(max_distance, goal_bias)` (rrt_connect.rs:86-95)
    pub fn new_connect(max_distance: f64, goal_bias: f64, checker: Arc<D>) -> Self {
        let mut p = Self::new(max_distance, goal_bias, checker);
        p.planner = TreePlanner::RrtConnect;
        p
    }

    pub fn with_options(mut self, options: HipOptions) -> Self {
        self.options = options;
        self
    }

    fn release(&mut self) {
        if !self.batch.is_null() {
            unsafe { ffi::oxhip_rrt_batch_destroy(self.batch) };
            self.batch = ptr::null_mut();
        }
    }

    /// the tree as (states, parent indices): `RRT::tree` (rrt.rs:61)
    pub fn tree(&self) -> Option<(Vec<RealVectorState>, Vec<i32>)> {
        let pd = self.problem_def.as_ref()?;
        if self.batch.is_null() {
            return None;
        }
        let dim = pd.space.dimension;
        let mut n = 0u32;
        unsafe { ffi::oxhip_rrt_batch_get_tree(self.batch, 0, ptr::null_mut(), ptr::null_mut(), 0, &mut n) };
        let mut flat = vec![0.0f64; n as usize * dim];
        let mut parents = vec![0i32; n as usize];
        let st = unsafe { ffi::oxhip_rrt_batch_get_tree(self.batch, 0, flat.as_mut_ptr(), parents.as_mut_ptr(), n, &mut n) };
        if st != ffi::OXHIP_OK {
            return None;
        }
        let states = flat.chunks(dim).map(|c| RealVectorState::new(c.to_vec())).collect();
        Some((states, parents))
    }

    /// The last solution, shortcut over its own waypoints on the device (`oxhip_rrt_batch_simplify_paths`: the cheapest
    /// chain of waypoints whose links pass the planner's own `check_motion`; `max_span` bounds how many waypoints a link
    /// may skip over, 0 = no bound).  Not part of the reference's surface.  `NoSolutionFound` when there is no solution.
    pub fn simplify_solution(&mut self, max_span: u32) -> Result<Path<RealVectorState>, PlanningError> {
        let pd = match (&self.problem_def, self.batch.is_null()) {
            (Some(pd), false) => pd.clone(),
            _ => return Err(PlanningError::PlannerUninitialised),
        };
        let rc = unsafe { ffi::oxhip_rrt_batch_simplify_paths(self.batch, max_span, 0) };
        if rc != ffi::OXHIP_OK {
            return Err(to_planning_error(rc));
        }
        let dim = pd.space.dimension;
        let mut offsets = [0u64; 2];
        let mut total = 0u64;
        unsafe { ffi::oxhip_rrt_batch_get_simplified_paths(self.batch, offsets.as_mut_ptr(), ptr::null_mut(), ptr::null_mut(), 0, &mut total) };
        if total == 0 {
            return Err(PlanningError::NoSolutionFound);
        }
        let mut flat = vec![0.0f64; total as usize * dim];
        let rc = unsafe { ffi::oxhip_rrt_batch_get_simplified_paths(self.batch, offsets.as_mut_ptr(), flat.as_mut_ptr(), ptr::null_mut(), total, &mut total) };
        if rc != ffi::OXHIP_OK {
            return Err(to_planning_error(rc));
        }
        Ok(Path(flat.chunks(dim).map(|c| RealVectorState::new(c.to_vec())).collect()))
    }

    /// Re-checks every edge of the tree against the batch's current obstacles (`oxhip_rrt_batch_revalidate_trees`): every
    /// node that a failed edge cuts off from the start is dropped, the rest keep their order, counters and the random
    /// stream stay, and a later `solve` continues from the pruned tree.  Returns the number of removed nodes.  RRT only:
    /// an RRTConnect or RRT* planner gets `NoSolutionFound` (the library refuses it with `OXHIP_ERR_BAD_ARG`).
    pub fn revalidate(&mut self) -> Result<u32, PlanningError> {
        if self.batch.is_null() {
            return Err(PlanningError::PlannerUninitialised);
        }
        let mut removed = 0u32;
        match unsafe { ffi::oxhip_rrt_batch_revalidate_trees(self.batch, &mut removed, ptr::null_mut()) } {
            ffi::OXHIP_OK => Ok(removed),
            rc => Err(to_planning_error(rc)),
        }
    }
}

impl<D: DeviceValidityChecker, G: DeviceGoal> Drop for HipRRT<D, G> {
    fn drop(&mut self) {
        self.release();
    }
}

impl<D: DeviceValidityChecker, G: DeviceGoal> Planner<RealVectorState, RealVectorStateSpace, G> for HipRRT<D, G> {
    /// `Planner::setup` (rrt.rs:140-156): stores the problem, clears the tree, pushes `start_states[0]`.
    ///
    /// Panics where the reference would (its `unwrap()` of the sampler's error at rrt.rs:183 for unbounded or
    /// zero-volume spaces) and when `validity_checker` disagrees with the description given to `new`.
    fn setup(&mut self, problem_def: Arc<Pd<G>>, validity_checker: Arc<dyn StateValidityChecker<RealVectorState>>) {
        self.release();
        let space = &problem_def.space;
        let dim = space.dimension;
        assert!(dim >= 1 && dim <= ffi::OXHIP_MAX_DIM, "HipRRT supports 1..=8 dimensions");
        let start = &problem_def.start_states[0];
        assert_eq!(start.values.len(), dim);

        let spheres = self.checker.spheres();
        let boxes = self.checker.boxes();

        // the trait object is all `setup` gets: make sure it is the checker that was described
        let mut probes: Vec<Vec<f64>> = vec![start.values.clone()];
        let mut lcg = 0x9E37_79B9_7F4A_7C15u64;
        for _ in 0..64 {
            let mut p = Vec::with_capacity(dim);
            for (lo, hi) in &space.bounds {
                lcg = lcg.wrapping_mul(6364136223846793005).wrapping_add(1442695040888963407);
                let u = (lcg >> 11) as f64 / (1u64 << 53) as f64;
                p.push(if lo.is_finite() && hi.is_finite() { lo + (hi - lo) * u } else { u });
            }
            probes.push(p);
        }
        for p in &probes {
            let state = RealVectorState::new(p.clone());
            assert_eq!(
                validity_checker.is_valid(&state),
                described_valid(&spheres, &boxes, p),
                "the StateValidityChecker given to setup() is not the one described to HipRRT::new (state {:?})",
                p
            );
        }

        let mut cfg: ffi::OxhipRrtConfig = unsafe { std::mem::zeroed() };
        cfg.struct_size = std::mem::size_of::<ffi::OxhipRrtConfig>() as u32;
        cfg.dim = dim as u32;
        for (k, (lo, hi)) in space.bounds.iter().enumerate() {
            cfg.bounds[2 * k] = *lo;
            cfg.bounds[2 * k + 1] = *hi;
        }
        cfg.max_distance = self.max_distance;
        cfg.goal_bias = self.goal_bias;
        cfg.lvs_fraction = fraction_of(space);
        cfg.n_problems = 1;
        cfg.max_nodes = self.options.max_nodes;
        cfg.stop_at_goal = 1;
        cfg.kernel = ffi::OXHIP_KERNEL_AUTO;
        cfg.seed = self.options.seed;
        cfg.first_problem_id = self.options.stream;
        cfg.device = self.options.device;
        cfg.space = ffi::OXHIP_SPACE_REAL_VECTOR;
        cfg.goal_sampler = match problem_def.goal.sampling() {
            GoalSampling::Centre => ffi::OXHIP_GOAL_SAMPLE_CENTRE,
            GoalSampling::UniformDisc => ffi::OXHIP_GOAL_SAMPLE_UNIFORM_DISC,
        };
        match self.planner {
            TreePlanner::Rrt => cfg.planner = ffi::OXHIP_PLANNER_RRT,
            TreePlanner::RrtConnect => cfg.planner = ffi::OXHIP_PLANNER_RRT_CONNECT,
            TreePlanner::RrtStar { search_radius } => {
                cfg.planner = ffi::OXHIP_PLANNER_RRT_STAR;
                cfg.search_radius = search_radius;
            }
        }
        let mut batch: *mut ffi::OxhipRrtBatch = ptr::null_mut();
        let st = unsafe { ffi::oxhip_rrt_batch_create(&cfg, &mut batch) };
        if st != ffi::OXHIP_OK {
            // UNBOUNDED / ZERO_VOLUME: the reference panics on the same condition at its first sample (rrt.rs:183)
            panic!("oxhip_rrt_batch_create failed with status {}: {}", st, last_error());
        }
        self.batch = batch;

        if !spheres.is_empty() {
            let centres = flatten(&spheres.iter().map(|(c, _)| c.clone()).collect::<Vec<_>>(), dim, "a sphere centre");
            let radii: Vec<f64> = spheres.iter().map(|(_, r)| *r).collect();
            let st = unsafe { ffi::oxhip_rrt_batch_set_spheres(self.batch, centres.as_ptr(), radii.as_ptr(), radii.len() as u32) };
            assert_eq!(st, ffi::OXHIP_OK, "set_spheres: {}", last_error());
        }
        if !boxes.is_empty() {
            let lo = flatten(&boxes.iter().map(|(l, _)| l.clone()).collect::<Vec<_>>(), dim, "a box corner");
            let hi = flatten(&boxes.iter().map(|(_, h)| h.clone()).collect::<Vec<_>>(), dim, "a box corner");
            let st = unsafe { ffi::oxhip_rrt_batch_set_boxes(self.batch, lo.as_ptr(), hi.as_ptr(), boxes.len() as u32) };
            assert_eq!(st, ffi::OXHIP_OK, "set_boxes: {}", last_error());
        }
        let (centre, radius) = problem_def.goal.ball();
        assert_eq!(centre.len(), dim);
        let st = unsafe { ffi::oxhip_rrt_batch_setup(self.batch, start.values.as_ptr(), centre.as_ptr(), &radius) };
        assert_eq!(st, ffi::OXHIP_OK, "setup: {}", last_error());
        self.problem_def = Some(problem_def);
    }

    /// `Planner::solve` (rrt.rs:158-227)
    fn solve(&mut self, timeout: Duration) -> Result<Path<RealVectorState>, PlanningError> {
        let pd = match (&self.problem_def, self.batch.is_null()) {
            (Some(pd), false) => pd.clone(),
            _ => return Err(PlanningError::PlannerUninitialised), // rrt.rs:160-163
        };
        if timeout.is_zero() {
            return Err(PlanningError::Timeout); // rrt.rs:172-174: elapsed() > 0 at the first check
        }
        let mut status = ffi::OXHIP_ERR_NO_SOLUTION_FOUND;
        let rc = unsafe { ffi::oxhip_rrt_batch_solve(self.batch, 1u64 << 40, timeout.as_secs_f64(), 0, &mut status) };
        if rc != ffi::OXHIP_OK {
            return Err(to_planning_error(rc));
        }
        if status != ffi::OXHIP_OK {
            return Err(to_planning_error(status));
        }
        let dim = pd.space.dimension;
        let mut len = 0u32;
        unsafe { ffi::oxhip_rrt_batch_get_path(self.batch, 0, ptr::null_mut(), 0, &mut len) };
        let mut flat = vec![0.0f64; len as usize * dim];
        let rc = unsafe { ffi::oxhip_rrt_batch_get_path(self.batch, 0, flat.as_mut_ptr(), len, &mut len) };
        if rc != ffi::OXHIP_OK {
            return Err(PlanningError::NoSolutionFound);
        }
        Ok(Path(flat.chunks(dim).map(|c| RealVectorState::new(c.to_vec())).collect()))
    }
}

/// GPU twin of `oxmpl::geometric::PRM` (prm.rs:48-57): same public fields, `construct_roadmap`,
/// `set_problem_definition`, and the `Planner` trait for the query.
pub struct HipPRM<D: DeviceValidityChecker, G: DeviceGoal> {
    pub timeout: f64,
    pub connection_radius: f64,
    /// construction also stops at this many milestones (a GPU fills seconds of wall clock with far too many)
    pub max_milestones: u32,
    pub options: HipOptions,
    checker: Arc<D>,
    problem_def: Option<Arc<Pd<G>>>,
    prm: *mut ffi::OxhipPrm,
    /// problems of the last `solve_batch` / `solve_batch_shortest`: what `simplify_batch` returns one entry each for
    last_batch_len: usize,
}

impl<D: DeviceValidityChecker, G: DeviceGoal> HipPRM<D, G> {
    /// `PRM::new(timeout, connection_radius)` (prm.rs:70-78) plus the typed obstacle description
    pub fn new(timeout: f64, connection_radius: f64, checker: Arc<D>) -> Self {
        HipPRM {
            timeout,
            connection_radius,
            max_milestones: 16_384,
            options: HipOptions::default(),
            checker,
            problem_def: None,
            prm: ptr::null_mut(),
            last_batch_len: 0,
        }
    }

    fn release(&mut self) {
        if !self.prm.is_null() {
            unsafe { ffi::oxhip_prm_destroy(self.prm) };
            self.prm = ptr::null_mut();
        }
    }

    /// `PRM::construct_roadmap` (prm.rs:96-154)
    pub fn construct_roadmap(&mut self) -> Result<(), PlanningError> {
        if self.prm.is_null() {
            return Err(PlanningError::PlannerUninitialised);
        }
        match unsafe { ffi::oxhip_prm_construct_roadmap(self.prm) } {
            ffi::OXHIP_OK => Ok(()),
            st => Err(to_planning_error(st)),
        }
    }

    /// `PRM::set_problem_definition` (prm.rs:88-90): a new start / goal on the roadmap already built
    pub fn set_problem_definition(&mut self, pd: Arc<Pd<G>>) {
        if !self.prm.is_null() {
            let (centre, radius) = pd.goal.ball();
            let st = unsafe { ffi::oxhip_prm_set_problem(self.prm, pd.start_states[0].values.as_ptr(), centre.as_ptr(), radius) };
            assert_eq!(st, ffi::OXHIP_OK, "set_problem: {}", last_error());
        }
        self.problem_def = Some(pd);
    }

    /// `PRM::get_roadmap` (prm.rs:82-84) as (states, per-node edge lists in the reference's order)
    pub fn get_roadmap(&self) -> Vec<(RealVectorState, Vec<usize>)> {
        let (pd, prm) = match (&self.problem_def, self.prm.is_null()) {
            (Some(pd), false) => (pd, self.prm),
            _ => return Vec::new(),
        };
        let dim = pd.space.dimension;
        let (mut n, mut entries, mut samples) = (0u32, 0u64, 0u64);
        unsafe { ffi::oxhip_prm_get_sizes(prm, &mut n, &mut entries, &mut samples) };
        let mut states = vec![0.0f64; n as usize * dim];
        let mut offsets = vec![0u64; n as usize + 1];
        let mut nbrs = vec![0u32; entries as usize];
        let st = unsafe { ffi::oxhip_prm_get_roadmap(prm, states.as_mut_ptr(), n, offsets.as_mut_ptr(), nbrs.as_mut_ptr(), entries) };
        if st != ffi::OXHIP_OK {
            return Vec::new();
        }
        (0..n as usize)
            .map(|i| {
                let edges = nbrs[offsets[i] as usize..offsets[i + 1] as usize].iter().map(|&v| v as usize).collect();
                (RealVectorState::new(states[i * dim..(i + 1) * dim].to_vec()), edges)
            })
            .collect()
    }

    /// Replaces the roadmap with the caller's, in `get_roadmap`'s shape (`oxhip_prm_set_roadmap`).  The library checks on the GPU
    /// that the edge lists are ascending and symmetric; `Err` carries its message (the rule and the lowest offending row) and the
    /// planner's roadmap is then unchanged.
    pub fn set_roadmap(&mut self, roadmap: &[(RealVectorState, Vec<usize>)]) -> Result<(), String> {
        let dim = match (&self.problem_def, self.prm.is_null()) {
            (Some(pd), false) => pd.space.dimension,
            _ => return Err("setup() was not called".to_string()),
        };
        let n = roadmap.len();
        let mut states = Vec::with_capacity(n * dim + 1);
        let mut offsets = vec![0u64; n + 1];
        let mut nbrs: Vec<u32> = Vec::new();
        for (i, (state, edges)) in roadmap.iter().enumerate() {
            if state.values.len() != dim {
                return Err(format!("milestone {} has {} coordinates, the space has {}", i, state.values.len(), dim));
            }
            states.extend_from_slice(&state.values);
            nbrs.extend(edges.iter().map(|&v| v.min(u32::MAX as usize) as u32));
            offsets[i + 1] = nbrs.len() as u64;
        }
        if states.is_empty() {
            states.push(0.0);
        }
        let nb = if nbrs.is_empty() { std::ptr::null() } else { nbrs.as_ptr() };
        match unsafe { ffi::oxhip_prm_set_roadmap(self.prm, states.as_ptr(), n as u32, offsets.as_ptr(), nb) } {
            ffi::OXHIP_OK => Ok(()),
            _ => Err(last_error()),
        }
    }

    /// Re-checks every milestone and edge of the roadmap against the handle's current obstacles (`oxhip_prm_revalidate`): an
    /// invalid milestone keeps its index and loses its edges.  Returns (valid per milestone, edge entries removed).
    pub fn revalidate(&mut self) -> Result<(Vec<bool>, u64), PlanningError> {
        if self.prm.is_null() {
            return Err(PlanningError::PlannerUninitialised);
        }
        let (mut n, mut entries, mut samples) = (0u32, 0u64, 0u64);
        unsafe { ffi::oxhip_prm_get_sizes(self.prm, &mut n, &mut entries, &mut samples) };
        let mut valid = vec![0u8; (n as usize).max(1)];
        let (mut bad, mut removed) = (0u32, 0u64);
        match unsafe { ffi::oxhip_prm_revalidate(self.prm, valid.as_mut_ptr(), &mut bad, &mut removed) } {
            ffi::OXHIP_OK => Ok((valid[..n as usize].iter().map(|&v| v != 0).collect(), removed)),
            st => Err(to_planning_error(st)),
        }
    }

    /// Adds up to `n_more` milestones to the roadmap as it stands -- built, planted or re-checked -- under the handle's current
    /// obstacles (`oxhip_prm_grow_roadmap`).  `new_stream: None` continues the planner's own sampler stream where
    /// `construct_roadmap` or the last grow stopped; a planted roadmap has no such position and needs `Some(stream id)`.
    /// Returns (milestones added, samples drawn); `Err` carries the library's message and the roadmap is then unchanged.
    pub fn grow_roadmap(&mut self, n_more: u32, max_samples: u64, new_stream: Option<u64>) -> Result<(u32, u64), String> {
        if self.prm.is_null() {
            return Err("setup() was not called".to_string());
        }
        let g = ffi::OxhipPrmGrowConfig {
            struct_size: std::mem::size_of::<ffi::OxhipPrmGrowConfig>() as u32,
            n_more,
            max_samples,
            flags: if new_stream.is_some() { ffi::OXHIP_PRM_GROW_NEW_STREAM } else { 0 },
            pad: 0,
            stream: new_stream.unwrap_or(0),
        };
        let (mut added, mut drawn) = (0u32, 0u64);
        match unsafe { ffi::oxhip_prm_grow_roadmap(self.prm, &g, &mut added, &mut drawn) } {
            ffi::OXHIP_OK => Ok((added, drawn)),
            _ => Err(last_error()),
        }
    }

    /// The roadmap's connected components (`oxhip_prm_components`): (label, size, n_components, largest_label, largest_size),
    /// `label[i]` being the lowest milestone index of i's component and `size[i]` its number of milestones.  Only the graph is read.
    #[allow(clippy::type_complexity)]
    pub fn components(&mut self) -> Result<(Vec<u32>, Vec<u32>, u32, u32, u32), PlanningError> {
        if self.prm.is_null() {
            return Err(PlanningError::PlannerUninitialised);
        }
        let (mut n, mut entries, mut samples) = (0u32, 0u64, 0u64);
        unsafe { ffi::oxhip_prm_get_sizes(self.prm, &mut n, &mut entries, &mut samples) };
        let mut label = vec![0u32; (n as usize).max(1)];
        let mut size = vec![0u32; (n as usize).max(1)];
        let (mut count, mut largest_label, mut largest_size) = (0u32, 0u32, 0u32);
        match unsafe {
            ffi::oxhip_prm_components(self.prm, label.as_mut_ptr(), size.as_mut_ptr(), n, &mut count, &mut largest_label, &mut largest_size)
        } {
            ffi::OXHIP_OK => {
                label.truncate(n as usize);
                size.truncate(n as usize);
                Ok((label, size, count, largest_label, largest_size))
            }
            st => Err(to_planning_error(st)),
        }
    }

    /// Removes milestones and renumbers the rest in their old order (`oxhip_prm_prune`): `invalid` drops the ones that are
    /// invalid now, `keep` the ones with a false entry; then, on the components of what is left, `min_size > 0` drops the
    /// components with fewer milestones and `largest` all but the largest.  No edge is re-checked.  Returns (new_index with
    /// -1 = dropped, milestones kept, edge entries removed); `Err` carries the library's message and the roadmap is then unchanged.
    pub fn prune(&mut self, invalid: bool, keep: Option<&[bool]>, min_size: u32, largest: bool) -> Result<(Vec<i32>, u32, u64), String> {
        if self.prm.is_null() {
            return Err("setup() was not called".to_string());
        }
        let (mut n, mut entries, mut samples) = (0u32, 0u64, 0u64);
        unsafe { ffi::oxhip_prm_get_sizes(self.prm, &mut n, &mut entries, &mut samples) };
        if keep.is_some_and(|k| k.len() != n as usize) {
            return Err("keep must hold one entry per milestone".to_string());
        }
        let mut flags = 0u32;
        if invalid {
            flags |= ffi::OXHIP_PRM_PRUNE_INVALID;
        }
        if keep.is_some() {
            flags |= ffi::OXHIP_PRM_PRUNE_MASK;
        }
        if min_size > 0 {
            flags |= ffi::OXHIP_PRM_PRUNE_MIN_SIZE;
        }
        if largest {
            flags |= ffi::OXHIP_PRM_PRUNE_LARGEST;
        }
        let c = ffi::OxhipPrmPruneConfig { struct_size: std::mem::size_of::<ffi::OxhipPrmPruneConfig>() as u32, flags, min_size, pad: 0 };
        let mask: Option<Vec<u8>> = keep.map(|k| if k.is_empty() { vec![0u8] } else { k.iter().map(|&b| b as u8).collect() });
        let mut new_index = vec![-1i32; (n as usize).max(1)];
        let (mut kept, mut removed) = (0u32, 0u64);
        let keep_ptr = mask.as_ref().map_or(std::ptr::null(), |m| m.as_ptr());
        match unsafe { ffi::oxhip_prm_prune(self.prm, &c, keep_ptr, new_index.as_mut_ptr(), &mut kept, &mut removed) } {
            ffi::OXHIP_OK => {
                new_index.truncate(n as usize);
                Ok((new_index, kept, removed))
            }
            _ => Err(last_error()),
        }
    }

    /// Many problem definitions on the roadmap already built, in one device call (`oxhip_prm_solve_batch`): per problem what
    /// `set_problem_definition` + `solve` would return, the breadth-first search included on the GPU.  The planner's own
    /// problem definition is left as it is.
    pub fn solve_batch(&mut self, problems: &[Arc<Pd<G>>], timeout: Duration) -> Vec<Result<Path<RealVectorState>, PlanningError>> {
        self.solve_batch_with(problems, timeout, false)
    }

    /// The same batch answered with shortest paths on the roadmap in the space's distance (`oxhip_prm_solve_batch_shortest`):
    /// the statuses are `solve_batch`'s, the paths are no longer than its fewest-hop ones.
    pub fn solve_batch_shortest(&mut self, problems: &[Arc<Pd<G>>], timeout: Duration) -> Vec<Result<Path<RealVectorState>, PlanningError>> {
        self.solve_batch_with(problems, timeout, true)
    }

    /// The answered paths of the last `solve_batch` / `solve_batch_shortest`, shortcut on the device
    /// (`oxhip_prm_batch_simplify_paths`): every edge is first cut into `subdivide` equal parts, then the cheapest chain of
    /// the resulting points whose links pass the planner's own `check_motion` is taken; `max_span` bounds a link in original
    /// edges, 0 = no bound.  One entry per problem of that batch, `None` for an unanswered one; `Err` carries the library's message.
    pub fn simplify_batch(&mut self, subdivide: u32, max_span: u32) -> Result<Vec<Option<Path<RealVectorState>>>, String> {
        let dim = match (&self.problem_def, self.prm.is_null()) {
            (Some(pd), false) => pd.space.dimension,
            _ => return Err("setup() was not called".to_string()),
        };
        if unsafe { ffi::oxhip_prm_batch_simplify_paths(self.prm, subdivide, max_span, 0) } != ffi::OXHIP_OK {
            return Err(last_error());
        }
        let q = self.last_batch_len;
        let mut offsets = vec![0u64; q + 1];
        let mut total = 0u64;
        if unsafe { ffi::oxhip_prm_batch_get_simplified_paths(self.prm, offsets.as_mut_ptr(), ptr::null_mut(), ptr::null_mut(), 0, &mut total) } != ffi::OXHIP_OK {
            return Err(last_error());
        }
        let mut flat = vec![0.0f64; (total as usize * dim).max(1)];
        let st = unsafe { ffi::oxhip_prm_batch_get_simplified_paths(self.prm, offsets.as_mut_ptr(), flat.as_mut_ptr(), ptr::null_mut(), total, &mut total) };
        if st != ffi::OXHIP_OK {
            return Err(last_error());
        }
        Ok((0..q)
            .map(|i| {
                let (a, b) = (offsets[i] as usize, offsets[i + 1] as usize);
                (b > a).then(|| Path(flat[a * dim..b * dim].chunks(dim).map(|c| RealVectorState::new(c.to_vec())).collect()))
            })
            .collect())
    }

    fn solve_batch_with(&mut self, problems: &[Arc<Pd<G>>], timeout: Duration, shortest: bool) -> Vec<Result<Path<RealVectorState>, PlanningError>> {
        let dim = match (&self.problem_def, self.prm.is_null()) {
            (Some(pd), false) => pd.space.dimension,
            _ => return problems.iter().map(|_| Err(PlanningError::PlannerUninitialised)).collect(), // prm.rs:229-236
        };
        let q = problems.len();
        let (mut starts, mut centres, mut radii) = (Vec::with_capacity(q * dim), Vec::with_capacity(q * dim), Vec::with_capacity(q));
        for pd in problems {
            let (centre, radius) = pd.goal.ball();
            assert!(pd.start_states[0].values.len() == dim && centre.len() == dim, "solve_batch: every problem must share the planner's space");
            starts.extend_from_slice(&pd.start_states[0].values);
            centres.extend_from_slice(&centre);
            radii.push(radius);
        }
        let mut status = vec![0i32; q.max(1)];
        let st = unsafe {
            if shortest {
                ffi::oxhip_prm_solve_batch_shortest(self.prm, q as u32, starts.as_ptr(), centres.as_ptr(), radii.as_ptr(), timeout.as_secs_f64(), 0, 0, status.as_mut_ptr())
            } else {
                ffi::oxhip_prm_solve_batch(self.prm, q as u32, starts.as_ptr(), centres.as_ptr(), radii.as_ptr(), timeout.as_secs_f64(), 0, status.as_mut_ptr())
            }
        };
        if st != ffi::OXHIP_OK {
            return problems.iter().map(|_| Err(to_planning_error(st))).collect();
        }
        self.last_batch_len = q; // the library accepted the batch; a refused call leaves its last batch, and this count, as they were
        let mut offsets = vec![0u64; q + 1];
        let mut total = 0u64;
        unsafe { ffi::oxhip_prm_batch_get_paths(self.prm, offsets.as_mut_ptr(), ptr::null_mut(), ptr::null_mut(), 0, &mut total) };
        let mut flat = vec![0.0f64; (total as usize * dim).max(1)];
        let st = unsafe { ffi::oxhip_prm_batch_get_paths(self.prm, offsets.as_mut_ptr(), ptr::null_mut(), flat.as_mut_ptr(), total, &mut total) };
        assert_eq!(st, ffi::OXHIP_OK, "batch_get_paths: {}", last_error());
        (0..q)
            .map(|i| {
                if status[i] != ffi::OXHIP_OK {
                    return Err(to_planning_error(status[i]));
                }
                let rows = &flat[offsets[i] as usize * dim..offsets[i + 1] as usize * dim];
                Ok(Path(rows.chunks(dim).map(|c| RealVectorState::new(c.to_vec())).collect()))
            })
            .collect()
    }
}

impl<D: DeviceValidityChecker, G: DeviceGoal> Drop for HipPRM<D, G> {
    fn drop(&mut self) {
        self.release();
    }
}

impl<D: DeviceValidityChecker, G: DeviceGoal> Planner<RealVectorState, RealVectorStateSpace, G> for HipPRM<D, G> {
    /// `Planner::setup` (prm.rs:217-225): stores problem and checker, clears the roadmap
    fn setup(&mut self, problem_def: Arc<Pd<G>>, validity_checker: Arc<dyn StateValidityChecker<RealVectorState>>) {
        self.release();
        let space = &problem_def.space;
        let dim = space.dimension;
        assert!(dim >= 1 && dim <= ffi::OXHIP_MAX_DIM, "HipPRM supports 1..=8 dimensions");
        let start = &problem_def.start_states[0];
        let spheres = self.checker.spheres();
        let boxes = self.checker.boxes();
        assert_eq!(
            validity_checker.is_valid(start),
            described_valid(&spheres, &boxes, &start.values),
            "the StateValidityChecker given to setup() is not the one described to HipPRM::new"
        );
        let mut cfg: ffi::OxhipPrmConfig = unsafe { std::mem::zeroed() };
        cfg.struct_size = std::mem::size_of::<ffi::OxhipPrmConfig>() as u32;
        cfg.dim = dim as u32;
        for (k, (lo, hi)) in space.bounds.iter().enumerate() {
            cfg.bounds[2 * k] = *lo;
            cfg.bounds[2 * k + 1] = *hi;
        }
        cfg.timeout = self.timeout;
        cfg.connection_radius = self.connection_radius;
        cfg.lvs_fraction = fraction_of(space);
        cfg.max_milestones = self.max_milestones;
        cfg.device = self.options.device;
        cfg.max_samples = 0;
        cfg.seed = self.options.seed;
        cfg.stream = self.options.stream;
        let mut prm: *mut ffi::OxhipPrm = ptr::null_mut();
        let st = unsafe { ffi::oxhip_prm_create(&cfg, &mut prm) };
        if st != ffi::OXHIP_OK {
            panic!("oxhip_prm_create failed with status {}: {}", st, last_error());
        }
        self.prm = prm;
        if !spheres.is_empty() {
            let centres = flatten(&spheres.iter().map(|(c, _)| c.clone()).collect::<Vec<_>>(), dim, "a sphere centre");
            let radii: Vec<f64> = spheres.iter().map(|(_, r)| *r).collect();
            let st = unsafe { ffi::oxhip_prm_set_spheres(self.prm, centres.as_ptr(), radii.as_ptr(), radii.len() as u32) };
            assert_eq!(st, ffi::OXHIP_OK, "set_spheres: {}", last_error());
        }
        if !boxes.is_empty() {
            let lo = flatten(&boxes.iter().map(|(l, _)| l.clone()).collect::<Vec<_>>(), dim, "a box corner");
            let hi = flatten(&boxes.iter().map(|(_, h)| h.clone()).collect::<Vec<_>>(), dim, "a box corner");
            let st = unsafe { ffi::oxhip_prm_set_boxes(self.prm, lo.as_ptr(), hi.as_ptr(), boxes.len() as u32) };
            assert_eq!(st, ffi::OXHIP_OK, "set_boxes: {}", last_error());
        }
        let (centre, radius) = problem_def.goal.ball();
        let st = unsafe { ffi::oxhip_prm_setup(self.prm, start.values.as_ptr(), centre.as_ptr(), radius) };
        assert_eq!(st, ffi::OXHIP_OK, "setup: {}", last_error());
        self.problem_def = Some(problem_def);
    }

    /// `Planner::solve` (prm.rs:227-307): the roadmap query
    fn solve(&mut self, timeout: Duration) -> Result<Path<RealVectorState>, PlanningError> {
        let pd = match (&self.problem_def, self.prm.is_null()) {
            (Some(pd), false) => pd.clone(),
            _ => return Err(PlanningError::PlannerUninitialised), // prm.rs:229-236
        };
        let dim = pd.space.dimension;
        let mut len = 0u32;
        let st = unsafe { ffi::oxhip_prm_solve(self.prm, timeout.as_secs_f64(), ptr::null_mut(), 0, &mut len) };
        if st != ffi::OXHIP_OK && st != ffi::OXHIP_ERR_CAPACITY {
            return Err(to_planning_error(st));
        }
        let mut flat = vec![0.0f64; len as usize * dim];
        let st = unsafe { ffi::oxhip_prm_solve(self.prm, timeout.as_secs_f64(), flat.as_mut_ptr(), len, &mut len) };
        if st != ffi::OXHIP_OK {
            return Err(to_planning_error(st));
        }
        Ok(Path(flat.chunks(dim).map(|c| RealVectorState::new(c.to_vec())).collect()))
    }
}

// ---- SO(3) (rrt_so3.hip): RRT over SO3StateSpace with forbidden cones.  Minimal for now: the configuration and the
// device's distance; a `Planner<SO3State, SO3StateSpace, G>` implementation in the shape of HipRRT is the next step.

/// `oxhip_rrt_config` of an SO(3) RRT batch of one problem: RRT::new(max_distance, goal_bias) over `space`.  The config's
/// bounds carry SO3StateSpace::bounds (centre quaternion, max_angle); `lvs_fraction` is the space's
/// longest_valid_segment_fraction (a private field of SO3StateSpace, 0.05 unless set).  Cones go in through
/// `oxhip_rrt_batch_set_spheres` with 4-wide centres.
pub fn so3_rrt_config(space: &SO3StateSpace, max_distance: f64, goal_bias: f64, lvs_fraction: f64, options: &HipOptions) -> ffi::OxhipRrtConfig {
    let (centre, max_angle) = &space.bounds;
    let mut bounds = [0.0f64; 2 * ffi::OXHIP_MAX_DIM];
    bounds[0] = centre.x;
    bounds[1] = centre.y;
    bounds[2] = centre.z;
    bounds[3] = centre.w;
    bounds[4] = *max_angle;
    ffi::OxhipRrtConfig {
        struct_size: ffi::OXHIP_RRT_CONFIG_SIZE as u32,
        dim: 4,
        bounds,
        max_distance,
        goal_bias,
        lvs_fraction,
        n_problems: 1,
        max_nodes: options.max_nodes,
        stop_at_goal: 1,
        kernel: ffi::OXHIP_KERNEL_AUTO,
        seed: options.seed,
        first_problem_id: options.stream,
        device: options.device,
        planner: ffi::OXHIP_PLANNER_RRT,
        search_radius: 0.0,
        space: ffi::OXHIP_SPACE_SO3,
        goal_sampler: ffi::OXHIP_GOAL_SAMPLE_CENTRE,
        debug_flags: 0,
        star_pool_share: 0,
        frozen_split: 0,
        reserved: 0,
    }
}

/// `oxhip_rrt_config` of an SO(2) RRT batch of one problem: RRT::new(max_distance, goal_bias) over `space`.  The config's
/// bounds carry SO2StateSpace::bounds (lo, hi), already clamped to [-PI, PI] by SO2StateSpace::new; `lvs_fraction` is the
/// space's longest_valid_segment_fraction (0.05 unless set).  States cross the boundary as their `value`, un-normalised
/// (SO2State::new normalises; the device takes what it is given).  Forbidden arcs go in through
/// `oxhip_rrt_batch_set_boxes` with 1-wide rows (min, max).
pub fn so2_rrt_config(space: &SO2StateSpace, max_distance: f64, goal_bias: f64, lvs_fraction: f64, options: &HipOptions) -> ffi::OxhipRrtConfig {
    let mut bounds = [0.0f64; 2 * ffi::OXHIP_MAX_DIM];
    bounds[0] = space.bounds.0;
    bounds[1] = space.bounds.1;
    ffi::OxhipRrtConfig {
        struct_size: ffi::OXHIP_RRT_CONFIG_SIZE as u32,
        dim: 1,
        bounds,
        max_distance,
        goal_bias,
        lvs_fraction,
        n_problems: 1,
        max_nodes: options.max_nodes,
        stop_at_goal: 1,
        kernel: ffi::OXHIP_KERNEL_AUTO,
        seed: options.seed,
        first_problem_id: options.stream,
        device: options.device,
        planner: ffi::OXHIP_PLANNER_RRT,
        search_radius: 0.0,
        space: ffi::OXHIP_SPACE_SO2,
        goal_sampler: ffi::OXHIP_GOAL_SAMPLE_CENTRE,
        debug_flags: 0,
        star_pool_share: 0,
        frozen_split: 0,
        reserved: 0,
    }
}

/// `oxhip_prm_config` of an SO(3) roadmap: PRM::new(timeout, connection_radius) over `space` (prm_so3.hip).  The bounds carry
/// SO3StateSpace::bounds (centre quaternion, max_angle) as in `so3_rrt_config`; cones go in through `oxhip_prm_set_spheres`
/// with 4-wide centres; the radius rule only (knn_k = 0).  `options.max_nodes` caps the milestones.
pub fn so3_prm_config(space: &SO3StateSpace, timeout: f64, connection_radius: f64, lvs_fraction: f64, options: &HipOptions) -> ffi::OxhipPrmConfig {
    let (centre, max_angle) = &space.bounds;
    let mut bounds = [0.0f64; 2 * ffi::OXHIP_MAX_DIM];
    bounds[0] = centre.x;
    bounds[1] = centre.y;
    bounds[2] = centre.z;
    bounds[3] = centre.w;
    bounds[4] = *max_angle;
    ffi::OxhipPrmConfig {
        struct_size: ffi::OXHIP_PRM_CONFIG_SIZE as u32,
        dim: 4,
        bounds,
        timeout,
        connection_radius,
        lvs_fraction,
        max_milestones: options.max_nodes,
        device: options.device,
        max_samples: 0,
        seed: options.seed,
        stream: options.stream,
        knn_k: 0,
        space: ffi::OXHIP_SPACE_SO3,
    }
}

/// SO3StateSpace::distance evaluated by the device (ox_acos: within one ulp of libm's acos), for checking a binding
pub fn so3_device_distance(device: i32, a: &SO3State, b: &SO3State) -> Result<f64, String> {
    let qa = [a.x, a.y, a.z, a.w];
    let qb = [b.x, b.y, b.z, b.w];
    let mut out = 0.0f64;
    let st = unsafe { ffi::oxhip_so3_op_batch(device, 0, qa.as_ptr(), qb.as_ptr(), ptr::null(), 1, &mut out) };
    if st != ffi::OXHIP_OK {
        return Err(last_error());
    }
    Ok(out)
}
