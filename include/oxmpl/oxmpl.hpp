// oxmpl.hpp -- C++17 host side of the drop-in boundary: the reference's trait surface for the RRT
// path, over the C ABI of include/oxmpl_hip.h.  Header-only; link with liboxmpl_hip.so.
//
// Names, argument meaning and error behaviour follow the reference (rossng/oxmpl, Rust):
//   oxmpl::base::RealVectorState            oxmpl/src/base/states/real_vector_state.rs:5-13
//   oxmpl::base::RealVectorStateSpace       oxmpl/src/base/spaces/real_vector_state_space.rs:65-129,137-186
//   oxmpl::base::StateValidityChecker       oxmpl/src/base/validity.rs:39-48
//   oxmpl::base::Goal / GoalRegion / GoalSampleableRegion   oxmpl/src/base/goal.rs:12-41
//   oxmpl::base::ProblemDefinition, Path    oxmpl/src/base/problem_definition.rs:16-20, planner.rs:16-17
//   oxmpl::base::PlanningError, StateSpaceError             oxmpl/src/base/error.rs:28-52,97-108
//   oxmpl::geometric::RRT                   oxmpl/src/geometric/planners/rrt.rs:53-83,140-227
//
// Rust's Result<T, E> becomes oxmpl::Result<T, E> (value or error, never an exception), Arc<T>
// becomes std::shared_ptr<T>.  Everything that computes runs on the GPU through the C ABI: there is
// no CPU fallback here.  A validity checker / goal must be device-describable (spheres + boxes, a
// ball); the planner refuses anything else with PlanningError::PlannerUninitialised at solve().
#pragma once

#include <chrono>
#include <cmath>
#include <limits>
#include <memory>
#include <string>
#include <utility>
#include <variant>
#include <vector>

#include "../oxmpl_hip.h"

namespace oxmpl {

template <typename T, typename E>
class Result {
  public:
    Result(T v) : v_(std::move(v)) {}                      // NOLINT: Ok(v)
    Result(E e) : v_(std::move(e)) {}                      // NOLINT: Err(e)
    bool is_ok() const { return v_.index() == 0; }
    bool is_err() const { return !is_ok(); }
    T& unwrap() { return std::get<0>(v_); }
    const T& unwrap() const { return std::get<0>(v_); }
    const E& err() const { return std::get<1>(v_); }

  private:
    std::variant<T, E> v_;
};

namespace base {

// ---- error.rs
enum class PlanningError { Timeout, NoSolutionFound, PlannerUninitialised, InvalidStartState, UnsampledStateSpace };
inline const char* to_string(PlanningError e) {
    switch (e) {
        case PlanningError::Timeout: return "No solution found within timeout.";
        case PlanningError::NoSolutionFound: return "No solution found.";
        case PlanningError::PlannerUninitialised: return "<Planner>.setup() was not called, thus Planner is uninitialised.";
        case PlanningError::InvalidStartState: return "Start state is not valid in the current StateSpace.";
        default: return "StateSpace is not sampled. Either Tree or Roadmap is empty.";
    }
}
struct StateSpaceError {
    enum Kind { DimensionMismatch, InvalidBound, ZeroDimensionUnbounded } kind;
    std::size_t expected = 0, found = 0;
    double lower = 0.0, upper = 0.0;
    bool operator==(const StateSpaceError& o) const { return kind == o.kind; }
};

// ---- states/real_vector_state.rs
struct RealVectorState {
    std::vector<double> values;
    RealVectorState() = default;
    explicit RealVectorState(std::vector<double> v) : values(std::move(v)) {}
    bool operator==(const RealVectorState& o) const { return values == o.values; }
};

// ---- spaces/real_vector_state_space.rs
class RealVectorStateSpace {
  public:
    std::size_t dimension = 0;
    std::vector<std::pair<double, double>> bounds;
    double longest_valid_segment_fraction = 0.05;

    // RealVectorStateSpace::new (rvss.rs:65-100): bounds == nullptr means unbounded in every dimension
    static Result<RealVectorStateSpace, StateSpaceError> create(std::size_t dimension,
                                                                const std::vector<std::pair<double, double>>* bounds_option) {
        RealVectorStateSpace s;
        s.dimension = dimension;
        if (bounds_option) {
            if (bounds_option->size() != dimension)
                return StateSpaceError{StateSpaceError::DimensionMismatch, dimension, bounds_option->size()};
            for (auto& b : *bounds_option)
                if (b.first >= b.second) return StateSpaceError{StateSpaceError::InvalidBound, 0, 0, b.first, b.second};
            s.bounds = *bounds_option;
        } else {
            if (dimension == 0) return StateSpaceError{StateSpaceError::ZeroDimensionUnbounded};
            const double inf = std::numeric_limits<double>::infinity();
            s.bounds.assign(dimension, {-inf, inf});
        }
        return s;
    }
    // rvss.rs:121-129
    void set_longest_valid_segment_fraction(double fraction) {
        if (fraction > 0.0 && fraction <= 1.0) longest_valid_segment_fraction = fraction;
        else if (fraction <= 0.0) longest_valid_segment_fraction = 0.0;
        else longest_valid_segment_fraction = 1.0;
    }
    // StateSpace::distance (rvss.rs:137-155), evaluated by the HIP library (oxhip_distance_batch)
    double distance(const RealVectorState& a, const RealVectorState& b, int device = 0) const {
        double out = std::numeric_limits<double>::quiet_NaN();
        if (a.values.size() == dimension && b.values.size() == dimension)
            (void)oxhip_distance_batch(device, (uint32_t)dimension, a.values.data(), b.values.data(), 1, &out);
        return out;
    }
    // StateSpace::interpolate (rvss.rs:161-186), evaluated by the HIP library (oxhip_interpolate_batch)
    void interpolate(const RealVectorState& from, const RealVectorState& to, double t, RealVectorState& out_state,
                     int device = 0) const {
        out_state.values.assign(dimension, std::numeric_limits<double>::quiet_NaN());
        (void)oxhip_interpolate_batch(device, (uint32_t)dimension, from.values.data(), to.values.data(), &t, 1,
                                      out_state.values.data());
    }
};

// ---- validity.rs: the reference's trait plus what a device-describable checker exposes
struct Sphere { std::vector<double> centre; double radius; };   // valid iff distance(centre, p) > radius
struct Box { std::vector<double> lo, hi; };                      // invalid iff lo_k <= p_k <= hi_k for all k
class StateValidityChecker {
  public:
    virtual ~StateValidityChecker() = default;
    // is_valid (validity.rs:39-48) is answered on the device from the description below
    virtual std::vector<Sphere> spheres() const { return {}; }
    virtual std::vector<Box> boxes() const { return {}; }
};

// ---- goal.rs: Goal / GoalRegion / GoalSampleableRegion collapsed onto the device-describable ball goal
class GoalSampleableRegion {
  public:
    virtual ~GoalSampleableRegion() = default;
    virtual RealVectorState target() const = 0;   // sample_goal() returns this state (README.md:160-162)
    virtual double radius() const = 0;            // is_satisfied(s) = distance(s, target) <= radius
};

// ---- problem_definition.rs / planner.rs
struct ProblemDefinition {
    std::shared_ptr<RealVectorStateSpace> space;
    std::vector<RealVectorState> start_states;
    std::shared_ptr<GoalSampleableRegion> goal;
};
struct Path { std::vector<RealVectorState> states; };   // Path(pub Vec<S>)

}  // namespace base

namespace geometric {

// RRT (rrt.rs:53-62) for one planning problem, grown on the GPU.
class RRT {
  public:
    double max_distance;
    double goal_bias;
    // build-defined termination and RNG key (the reference stops on wall clock only and cannot be seeded)
    uint32_t max_nodes = 10000;
    uint64_t seed = 0;
    uint64_t problem_id = 0;
    int device = 0;

    RRT(double max_distance_, double goal_bias_) : max_distance(max_distance_), goal_bias(goal_bias_) {}  // rrt.rs:75-83
    virtual ~RRT() { reset(); }
    RRT(const RRT&) = delete;
    RRT& operator=(const RRT&) = delete;

    // Planner::setup (rrt.rs:140-156)
    void setup(std::shared_ptr<base::ProblemDefinition> problem_def, std::shared_ptr<base::StateValidityChecker> validity_checker) {
        reset();
        pd_ = std::move(problem_def);
        vc_ = std::move(validity_checker);
        last_status_ = OXHIP_OK;
        if (!pd_ || !vc_ || !pd_->space || !pd_->goal || pd_->start_states.empty()) { last_status_ = OXHIP_ERR_BAD_ARG; return; }
        const auto& sp = *pd_->space;
        oxhip_rrt_config cfg{};
        cfg.struct_size = sizeof cfg;
        cfg.dim = (uint32_t)sp.dimension;
        for (std::size_t k = 0; k < sp.bounds.size() && k < OXHIP_MAX_DIM; ++k) {
            cfg.bounds[2 * k] = sp.bounds[k].first;
            cfg.bounds[2 * k + 1] = sp.bounds[k].second;
        }
        cfg.max_distance = max_distance;
        cfg.goal_bias = goal_bias;
        cfg.lvs_fraction = sp.longest_valid_segment_fraction;
        cfg.n_problems = 1;
        cfg.max_nodes = max_nodes;
        cfg.stop_at_goal = 1;
        cfg.kernel = OXHIP_KERNEL_AUTO;
        cfg.seed = seed;
        cfg.first_problem_id = problem_id;
        cfg.device = device;
        cfg.planner = planner_kind();
        cfg.search_radius = search_radius_value();
        if ((last_status_ = oxhip_rrt_batch_create(&cfg, &batch_)) != OXHIP_OK) return;
        std::vector<double> c, r, lo, hi;
        for (auto& s : vc_->spheres()) { c.insert(c.end(), s.centre.begin(), s.centre.end()); r.push_back(s.radius); }
        for (auto& b : vc_->boxes()) { lo.insert(lo.end(), b.lo.begin(), b.lo.end()); hi.insert(hi.end(), b.hi.begin(), b.hi.end()); }
        if (!r.empty() && (last_status_ = oxhip_rrt_batch_set_spheres(batch_, c.data(), r.data(), (uint32_t)r.size())) != OXHIP_OK) return;
        if (!lo.empty() && (last_status_ = oxhip_rrt_batch_set_boxes(batch_, lo.data(), hi.data(), (uint32_t)(lo.size() / sp.dimension))) != OXHIP_OK) return;
        const auto target = pd_->goal->target();
        const double radius = pd_->goal->radius();
        last_status_ = oxhip_rrt_batch_setup(batch_, pd_->start_states[0].values.data(), target.values.data(), &radius);
    }

    // Planner::solve (rrt.rs:158-227)
    Result<base::Path, base::PlanningError> solve(std::chrono::duration<double> timeout) {
        if (!batch_ || last_status_ != OXHIP_OK) return base::PlanningError::PlannerUninitialised;  // rrt.rs:160-163
        // rrt.rs:172-174: `start_time.elapsed() > timeout` holds at the first check for a zero Duration (Rust's Duration has
        // no negative values or NaN: both are treated like zero here)
        if (!(timeout.count() > 0.0)) return base::PlanningError::Timeout;
        int32_t st = OXHIP_ERR_NO_SOLUTION_FOUND;
        last_status_ = oxhip_rrt_batch_solve(batch_, 1ull << 40, timeout.count(), 0, &st);
        if (last_status_ == OXHIP_ERR_PLANNER_UNINITIALISED) return base::PlanningError::PlannerUninitialised;
        if (last_status_ != OXHIP_OK) return base::PlanningError::NoSolutionFound;
        if (st == OXHIP_ERR_TIMEOUT) return base::PlanningError::Timeout;
        if (st != OXHIP_OK) return base::PlanningError::NoSolutionFound;
        uint32_t len = 0;
        (void)oxhip_rrt_batch_get_path(batch_, 0, nullptr, 0, &len);
        const std::size_t dim = pd_->space->dimension;
        std::vector<double> flat((std::size_t)len * dim);
        if ((last_status_ = oxhip_rrt_batch_get_path(batch_, 0, flat.data(), len, &len)) != OXHIP_OK)
            return base::PlanningError::NoSolutionFound;
        base::Path path;
        for (uint32_t i = 0; i < len; ++i)
            path.states.emplace_back(std::vector<double>(flat.begin() + i * dim, flat.begin() + (i + 1) * dim));
        return path;
    }

    // The last solution, shortcut over its own waypoints on the device (oxhip_rrt_batch_simplify_paths: the cheapest chain of
    // waypoints whose links pass the planner's own check_motion; max_span bounds how many waypoints a link may skip over, 0 =
    // no bound).  Not part of the reference's surface.  NoSolutionFound when there is no solution.
    Result<base::Path, base::PlanningError> simplify_solution(uint32_t max_span = 0) {
        if (!batch_ || last_status_ != OXHIP_OK) return base::PlanningError::PlannerUninitialised;
        const int32_t st = oxhip_rrt_batch_simplify_paths(batch_, max_span, 0);
        if (st == OXHIP_ERR_PLANNER_UNINITIALISED) return base::PlanningError::PlannerUninitialised;
        if (st != OXHIP_OK) return base::PlanningError::NoSolutionFound;
        uint64_t off[2] = {0, 0}, total = 0;
        (void)oxhip_rrt_batch_get_simplified_paths(batch_, off, nullptr, nullptr, 0, &total);
        if (total == 0) return base::PlanningError::NoSolutionFound;
        const std::size_t dim = pd_->space->dimension;
        std::vector<double> flat((std::size_t)total * dim);
        if (oxhip_rrt_batch_get_simplified_paths(batch_, off, flat.data(), nullptr, total, &total) != OXHIP_OK)
            return base::PlanningError::NoSolutionFound;
        base::Path path;
        for (uint64_t i = 0; i < total; ++i)
            path.states.emplace_back(std::vector<double>(flat.begin() + i * dim, flat.begin() + (i + 1) * dim));
        return path;
    }

    // Re-checks every edge of the tree against the obstacles of `checker` as they are now (oxhip_rrt_batch_revalidate_trees):
    // every node that a failed edge cuts off from the start is dropped, the rest keep their order, counters and the random
    // stream stay, and a later solve() continues from the pruned tree.  Returns the number of removed nodes.  RRT only:
    // an RRTConnect or RRTStar planner is refused (NoSolutionFound; oxhip_last_error_string() says why).
    Result<uint32_t, base::PlanningError> revalidate(const std::shared_ptr<base::StateValidityChecker>& checker) {
        if (!batch_ || !pd_ || !checker || last_status_ != OXHIP_OK) return base::PlanningError::PlannerUninitialised;
        std::vector<double> c, r, lo, hi;
        for (auto& s : checker->spheres()) { c.insert(c.end(), s.centre.begin(), s.centre.end()); r.push_back(s.radius); }
        for (auto& b : checker->boxes()) { lo.insert(lo.end(), b.lo.begin(), b.lo.end()); hi.insert(hi.end(), b.hi.begin(), b.hi.end()); }
        int32_t st = oxhip_rrt_batch_set_spheres(batch_, c.data(), r.data(), (uint32_t)r.size());
        if (st == OXHIP_OK) st = oxhip_rrt_batch_set_boxes(batch_, lo.data(), hi.data(), (uint32_t)(lo.size() / pd_->space->dimension));
        if (st != OXHIP_OK) return base::PlanningError::NoSolutionFound;
        vc_ = checker;
        return revalidate();
    }
    Result<uint32_t, base::PlanningError> revalidate() {
        if (!batch_ || last_status_ != OXHIP_OK) return base::PlanningError::PlannerUninitialised;
        uint32_t removed = 0;
        const int32_t st = oxhip_rrt_batch_revalidate_trees(batch_, &removed, nullptr);
        if (st == OXHIP_ERR_PLANNER_UNINITIALISED) return base::PlanningError::PlannerUninitialised;
        if (st != OXHIP_OK) return base::PlanningError::NoSolutionFound;
        return removed;
    }

    // batched StateValidityChecker::is_valid / RRT::check_motion on the device (test helpers)
    bool is_valid(const base::RealVectorState& s) const {
        uint8_t ok = 0;
        if (batch_) (void)oxhip_rrt_batch_is_valid(batch_, s.values.data(), 1, &ok);
        return ok != 0;
    }
    uint32_t num_nodes() const {
        uint32_t n = 0;
        if (batch_) (void)oxhip_rrt_batch_get_counts(batch_, nullptr, &n, nullptr, nullptr, nullptr, nullptr);
        return n;
    }
    int32_t last_status() const { return last_status_; }

  protected:
    virtual uint32_t planner_kind() const { return OXHIP_PLANNER_RRT; }
    virtual double search_radius_value() const { return 0.0; }
    oxhip_rrt_batch* batch() const { return batch_; }

  private:
    void reset() {
        if (batch_) (void)oxhip_rrt_batch_destroy(batch_);
        batch_ = nullptr;
    }
    oxhip_rrt_batch* batch_ = nullptr;
    std::shared_ptr<base::ProblemDefinition> pd_;
    std::shared_ptr<base::StateValidityChecker> vc_;
    int32_t last_status_ = OXHIP_ERR_PLANNER_UNINITIALISED;
};

// RRTConnect (rrt_connect.rs:49-95): same Planner surface, two trees grown towards each other.
class RRTConnect : public RRT {
  public:
    RRTConnect(double max_distance_, double goal_bias_) : RRT(max_distance_, goal_bias_) {}  // rrt_connect.rs:86-95

  protected:
    uint32_t planner_kind() const override { return OXHIP_PLANNER_RRT_CONNECT; }
};

// RRTStar (rrt_star.rs:39-52): RRT with choose-parent and rewire inside `search_radius`.
class RRTStar : public RRT {
  public:
    double search_radius;
    RRTStar(double max_distance_, double goal_bias_, double search_radius_)   // rrt_star.rs:68-77
        : RRT(max_distance_, goal_bias_), search_radius(search_radius_) {}

    // Node::cost (rrt_star.rs:26) of every node, in node order
    std::vector<double> costs() const {
        uint32_t n = 0;
        if (!batch() || oxhip_rrt_batch_get_costs(batch(), 0, nullptr, 0, &n) != OXHIP_OK) return {};
        std::vector<double> c(n);
        if (oxhip_rrt_batch_get_costs(batch(), 0, c.data(), n, &n) != OXHIP_OK) return {};
        return c;
    }

  protected:
    uint32_t planner_kind() const override { return OXHIP_PLANNER_RRT_STAR; }
    double search_radius_value() const override { return search_radius; }
};

// PRM (prm.rs:48-57): roadmap built and queried on the GPU.
class PRM {
  public:
    double timeout;             // seconds of roadmap construction (prm.rs:50); the device path also stops at max_milestones
    double connection_radius;   // prm.rs:52
    // build-defined termination and RNG key
    uint32_t max_milestones = 16384;
    uint64_t max_samples = 0;   // 0 = unlimited
    uint64_t seed = 0;
    uint64_t stream = 0;
    int device = 0;

    PRM(double timeout_, double connection_radius_) : timeout(timeout_), connection_radius(connection_radius_) {}  // prm.rs:70-78
    ~PRM() { reset(); }
    PRM(const PRM&) = delete;
    PRM& operator=(const PRM&) = delete;

    // Planner::setup (prm.rs:217-225)
    void setup(std::shared_ptr<base::ProblemDefinition> problem_def, std::shared_ptr<base::StateValidityChecker> validity_checker) {
        reset();
        pd_ = std::move(problem_def);
        last_status_ = OXHIP_OK;
        if (!pd_ || !validity_checker || !pd_->space || !pd_->goal || pd_->start_states.empty()) { last_status_ = OXHIP_ERR_BAD_ARG; return; }
        const auto& sp = *pd_->space;
        oxhip_prm_config cfg{};
        cfg.struct_size = sizeof cfg;
        cfg.dim = (uint32_t)sp.dimension;
        for (std::size_t k = 0; k < sp.bounds.size() && k < OXHIP_MAX_DIM; ++k) {
            cfg.bounds[2 * k] = sp.bounds[k].first;
            cfg.bounds[2 * k + 1] = sp.bounds[k].second;
        }
        cfg.timeout = timeout;
        cfg.connection_radius = connection_radius;
        cfg.lvs_fraction = sp.longest_valid_segment_fraction;
        cfg.max_milestones = max_milestones;
        cfg.max_samples = max_samples;
        cfg.seed = seed;
        cfg.stream = stream;
        cfg.device = device;
        if ((last_status_ = oxhip_prm_create(&cfg, &prm_)) != OXHIP_OK) return;
        std::vector<double> c, r, lo, hi;
        for (auto& s : validity_checker->spheres()) { c.insert(c.end(), s.centre.begin(), s.centre.end()); r.push_back(s.radius); }
        for (auto& b : validity_checker->boxes()) { lo.insert(lo.end(), b.lo.begin(), b.lo.end()); hi.insert(hi.end(), b.hi.begin(), b.hi.end()); }
        if (!r.empty() && (last_status_ = oxhip_prm_set_spheres(prm_, c.data(), r.data(), (uint32_t)r.size())) != OXHIP_OK) return;
        if (!lo.empty() && (last_status_ = oxhip_prm_set_boxes(prm_, lo.data(), hi.data(), (uint32_t)(lo.size() / sp.dimension))) != OXHIP_OK) return;
        const auto target = pd_->goal->target();
        last_status_ = oxhip_prm_setup(prm_, pd_->start_states[0].values.data(), target.values.data(), pd_->goal->radius());
    }

    // PRM::set_problem_definition (prm.rs:88-90): keeps the roadmap
    void set_problem_definition(std::shared_ptr<base::ProblemDefinition> pd) {
        pd_ = std::move(pd);
        if (prm_ && pd_ && pd_->goal && !pd_->start_states.empty()) {
            const auto target = pd_->goal->target();
            last_status_ = oxhip_prm_set_problem(prm_, pd_->start_states[0].values.data(), target.values.data(), pd_->goal->radius());
        }
    }

    // PRM::construct_roadmap (prm.rs:96-154)
    Result<bool, base::PlanningError> construct_roadmap() {
        if (!prm_ || last_status_ != OXHIP_OK) return base::PlanningError::PlannerUninitialised;  // prm.rs:97-104
        last_status_ = oxhip_prm_construct_roadmap(prm_);
        if (last_status_ != OXHIP_OK) return base::PlanningError::PlannerUninitialised;
        return true;
    }

    // Planner::solve (prm.rs:227-307)
    Result<base::Path, base::PlanningError> solve(std::chrono::duration<double> timeout_) {
        if (!prm_) return base::PlanningError::PlannerUninitialised;
        uint32_t len = 0;
        int32_t st = oxhip_prm_solve(prm_, timeout_.count(), nullptr, 0, &len);
        if (st != OXHIP_OK) return to_error(st);
        const std::size_t dim = pd_->space->dimension;
        std::vector<double> flat((std::size_t)len * dim);
        if ((st = oxhip_prm_solve(prm_, timeout_.count(), flat.data(), len, &len)) != OXHIP_OK) return to_error(st);
        base::Path path;
        for (uint32_t i = 0; i < len; ++i)
            path.states.emplace_back(std::vector<double>(flat.begin() + i * dim, flat.begin() + (i + 1) * dim));
        return path;
    }

    // Many problem definitions on the roadmap already built, in one device call (oxhip_prm_solve_batch: start connections, goal
    // test, breadth-first search and path extraction on the GPU): per problem what set_problem_definition + solve would return.
    // The planner's own problem definition is left as it is.  Every problem must share the planner's space.
    std::vector<Result<base::Path, base::PlanningError>> solve_batch(const std::vector<std::shared_ptr<base::ProblemDefinition>>& problems,
                                                                     std::chrono::duration<double> timeout_) {
        return solve_batch_with(problems, timeout_, false);
    }

    // The same batch answered with shortest paths on the roadmap in the space's distance (oxhip_prm_solve_batch_shortest): the
    // statuses are solve_batch's, the paths are no longer than its fewest-hop ones.
    std::vector<Result<base::Path, base::PlanningError>> solve_batch_shortest(const std::vector<std::shared_ptr<base::ProblemDefinition>>& problems,
                                                                              std::chrono::duration<double> timeout_) {
        return solve_batch_with(problems, timeout_, true);
    }

  private:
    std::vector<Result<base::Path, base::PlanningError>> solve_batch_with(const std::vector<std::shared_ptr<base::ProblemDefinition>>& problems,
                                                                          std::chrono::duration<double> timeout_, bool shortest) {
        std::vector<Result<base::Path, base::PlanningError>> out;
        out.reserve(problems.size());
        const std::size_t q = problems.size();
        if (!prm_ || !pd_) {
            for (std::size_t i = 0; i < q; ++i) out.emplace_back(base::PlanningError::PlannerUninitialised);
            return out;
        }
        const std::size_t dim = pd_->space->dimension;
        std::vector<double> starts, centres, radii;
        for (const auto& pd : problems) {
            const bool fits = pd && pd->goal && !pd->start_states.empty() && pd->start_states[0].values.size() == dim;
            const auto target = fits ? pd->goal->target() : pd_->goal->target();
            if (!fits || target.values.size() != dim) {
                for (std::size_t i = 0; i < q; ++i) out.emplace_back(base::PlanningError::PlannerUninitialised);
                return out;
            }
            starts.insert(starts.end(), pd->start_states[0].values.begin(), pd->start_states[0].values.end());
            centres.insert(centres.end(), target.values.begin(), target.values.end());
            radii.push_back(pd->goal->radius());
        }
        std::vector<int32_t> status(q ? q : 1);
        int32_t st = shortest ? oxhip_prm_solve_batch_shortest(prm_, (uint32_t)q, starts.data(), centres.data(), radii.data(), timeout_.count(), 0, 0,
                                                               status.data())
                              : oxhip_prm_solve_batch(prm_, (uint32_t)q, starts.data(), centres.data(), radii.data(), timeout_.count(), 0, status.data());
        if (st == OXHIP_OK) last_batch_ = q;   // (a refused call leaves the library's last batch, and so this count, as they were)
        std::vector<uint64_t> off(q + 1);
        uint64_t total = 0;
        if (st == OXHIP_OK) st = oxhip_prm_batch_get_paths(prm_, off.data(), nullptr, nullptr, 0, &total);
        std::vector<double> flat((std::size_t)total * dim + 1);
        if (st == OXHIP_OK) st = oxhip_prm_batch_get_paths(prm_, off.data(), nullptr, flat.data(), total, &total);
        for (std::size_t i = 0; i < q; ++i) {
            if (st != OXHIP_OK || status[i] != OXHIP_OK) {
                out.emplace_back(to_error(st != OXHIP_OK ? st : status[i]));
                continue;
            }
            base::Path path;
            for (uint64_t r = off[i]; r < off[i + 1]; ++r)
                path.states.emplace_back(std::vector<double>(flat.begin() + r * dim, flat.begin() + (r + 1) * dim));
            out.emplace_back(std::move(path));
        }
        return out;
    }

  public:
    // The planner's own StateValidityChecker and check_motion on the device, against the obstacles as they are now
    // (oxhip_prm_is_valid / oxhip_prm_check_motion); false before setup().
    bool is_valid(const base::RealVectorState& state) {
        uint8_t ok = 0;
        if (!prm_ || !pd_ || state.values.size() != pd_->space->dimension) return false;
        return oxhip_prm_is_valid(prm_, state.values.data(), 1, &ok) == OXHIP_OK && ok != 0;
    }
    bool check_motion(const base::RealVectorState& from, const base::RealVectorState& to) {
        uint8_t ok = 0;
        if (!prm_ || !pd_ || from.values.size() != pd_->space->dimension || to.values.size() != from.values.size()) return false;
        return oxhip_prm_check_motion(prm_, from.values.data(), to.values.data(), 1, &ok) == OXHIP_OK && ok != 0;
    }
    // The answered paths of the last solve_batch / solve_batch_shortest, shortcut on the device
    // (oxhip_prm_batch_simplify_paths): every edge is first cut into `subdivide` equal parts, then the cheapest chain of the
    // resulting points whose links pass the planner's own check_motion is taken; max_span bounds a link in original edges,
    // 0 = no bound.  Per problem of that batch the simplified path, or the batch's own error for one it did not answer.  A
    // refused call (no batch, subdivide outside 1..256, a path too large) gives every entry that error and leaves the planner
    // usable; last_simplify_status() holds the library's status either way (an empty result with OXHIP_OK: an empty batch).
    std::vector<Result<base::Path, base::PlanningError>> simplify_batch(uint32_t subdivide = 1, uint32_t max_span = 0) {
        const std::size_t n_problems = last_batch_;   // the library's last accepted batch: what its getters write
        std::vector<Result<base::Path, base::PlanningError>> out;
        out.reserve(n_problems);
        int32_t st = prm_ && pd_ ? oxhip_prm_batch_simplify_paths(prm_, subdivide, max_span, 0) : (int32_t)OXHIP_ERR_PLANNER_UNINITIALISED;
        simplify_status_ = st;
        std::vector<int32_t> status(n_problems ? n_problems : 1);
        if (st == OXHIP_OK) st = oxhip_prm_batch_get_results(prm_, status.data(), nullptr, nullptr, nullptr, nullptr);
        std::vector<uint64_t> off(n_problems + 1);
        uint64_t total = 0;
        if (st == OXHIP_OK) st = oxhip_prm_batch_get_simplified_paths(prm_, off.data(), nullptr, nullptr, 0, &total);
        const std::size_t dim = pd_ ? pd_->space->dimension : 0;
        std::vector<double> flat((std::size_t)total * dim + 1);
        if (st == OXHIP_OK) st = oxhip_prm_batch_get_simplified_paths(prm_, off.data(), flat.data(), nullptr, total, &total);
        for (std::size_t i = 0; i < n_problems; ++i) {
            if (st != OXHIP_OK || status[i] != OXHIP_OK) {
                out.emplace_back(to_error(st != OXHIP_OK ? st : status[i]));
                continue;
            }
            base::Path path;
            for (uint64_t r = off[i]; r < off[i + 1]; ++r)
                path.states.emplace_back(std::vector<double>(flat.begin() + r * dim, flat.begin() + (r + 1) * dim));
            out.emplace_back(std::move(path));
        }
        if (simplify_status_ == OXHIP_OK) simplify_status_ = st;
        return out;
    }
    int32_t last_simplify_status() const { return simplify_status_; }

    // PRM::get_roadmap (prm.rs:82-84): milestone count and, per node, its `edges`
    uint32_t num_milestones() const {
        uint32_t n = 0;
        if (prm_) (void)oxhip_prm_get_sizes(prm_, &n, nullptr, nullptr);
        return n;
    }
    struct Roadmap { std::vector<base::RealVectorState> states; std::vector<std::vector<uint32_t>> edges; };
    Roadmap get_roadmap() const {
        Roadmap rm;
        if (!prm_) return rm;
        uint32_t n = 0;
        uint64_t e = 0;
        (void)oxhip_prm_get_sizes(prm_, &n, &e, nullptr);
        const std::size_t dim = pd_->space->dimension;
        std::vector<double> flat((std::size_t)n * dim);
        std::vector<uint64_t> off((std::size_t)n + 1);
        std::vector<uint32_t> nb((std::size_t)e);
        if (oxhip_prm_get_roadmap(prm_, flat.data(), n, off.data(), nb.data(), e) != OXHIP_OK) return rm;
        for (uint32_t i = 0; i < n; ++i) {
            rm.states.emplace_back(std::vector<double>(flat.begin() + i * dim, flat.begin() + (i + 1) * dim));
            rm.edges.emplace_back(nb.begin() + off[i], nb.begin() + off[i + 1]);
        }
        return rm;
    }
    // Replaces the roadmap with `rm` (oxhip_prm_set_roadmap): the library checks on the GPU that the edge lists are ascending
    // and symmetric.  A refused roadmap returns false and leaves the planner's own as it was and the planner usable
    // (last_status() stays OXHIP_OK); last_set_roadmap_status() holds OXHIP_ERR_BAD_ARG / _CAPACITY and
    // oxhip_last_error_string() the rule and the row.
    bool set_roadmap(const Roadmap& rm) {
        if (!prm_ || !pd_ || rm.states.size() != rm.edges.size()) return false;
        const std::size_t dim = pd_->space->dimension, n = rm.states.size();
        std::vector<double> flat;
        std::vector<uint64_t> off(n + 1, 0);
        std::vector<uint32_t> nb;
        for (std::size_t i = 0; i < n; ++i) {
            if (rm.states[i].values.size() != dim) return false;
            flat.insert(flat.end(), rm.states[i].values.begin(), rm.states[i].values.end());
            nb.insert(nb.end(), rm.edges[i].begin(), rm.edges[i].end());
            off[i + 1] = nb.size();
        }
        if (flat.empty()) flat.push_back(0.0);
        set_roadmap_status_ = oxhip_prm_set_roadmap(prm_, flat.data(), (uint32_t)n, off.data(), nb.empty() ? nullptr : nb.data());
        if (set_roadmap_status_ != OXHIP_OK && set_roadmap_status_ != OXHIP_ERR_BAD_ARG && set_roadmap_status_ != OXHIP_ERR_CAPACITY)
            last_status_ = set_roadmap_status_;   // (a refusal leaves the planner as it was; anything else is the planner's error)
        return set_roadmap_status_ == OXHIP_OK;
    }
    int32_t last_set_roadmap_status() const { return set_roadmap_status_; }
    // Re-checks every milestone and edge against the obstacles of `checker` as they are now (oxhip_prm_revalidate); an
    // invalid milestone keeps its index and loses its edges.  valid[i] per milestone, and the edge entries removed.
    struct Revalidation { std::vector<uint8_t> valid; uint64_t removed_entries = 0; };
    Result<Revalidation, base::PlanningError> revalidate(const std::shared_ptr<base::StateValidityChecker>& checker) {
        if (!prm_ || !pd_ || !checker) return base::PlanningError::PlannerUninitialised;
        std::vector<double> c, r, lo, hi;
        for (auto& s : checker->spheres()) { c.insert(c.end(), s.centre.begin(), s.centre.end()); r.push_back(s.radius); }
        for (auto& b : checker->boxes()) { lo.insert(lo.end(), b.lo.begin(), b.lo.end()); hi.insert(hi.end(), b.hi.begin(), b.hi.end()); }
        int32_t st = oxhip_prm_set_spheres(prm_, c.data(), r.data(), (uint32_t)r.size());
        if (st == OXHIP_OK) st = oxhip_prm_set_boxes(prm_, lo.data(), hi.data(), (uint32_t)(lo.size() / pd_->space->dimension));
        if (st != OXHIP_OK) return to_error(st);
        return revalidate();
    }
    Result<Revalidation, base::PlanningError> revalidate() {
        if (!prm_) return base::PlanningError::PlannerUninitialised;
        Revalidation out;
        out.valid.assign(num_milestones(), 0);
        const int32_t st = oxhip_prm_revalidate(prm_, out.valid.empty() ? nullptr : out.valid.data(), nullptr, &out.removed_entries);
        if (st != OXHIP_OK) return to_error(st);
        return out;
    }
    // Adds up to n_more milestones to the roadmap as it stands -- built, planted or re-checked -- under the obstacles as they
    // are now (oxhip_prm_grow_roadmap).  `new_stream` null continues the planner's own sampler stream where construct_roadmap
    // or the last grow stopped; a planted roadmap has no such position and needs a stream id.  A refused argument
    // (OXHIP_ERR_BAD_ARG / _CAPACITY, kept in last_grow_status(), the text in oxhip_last_error_string()) comes back as
    // NoSolutionFound and leaves the roadmap as it was.
    struct Growth { uint32_t added = 0; uint64_t samples_drawn = 0; };
    Result<Growth, base::PlanningError> grow_roadmap(uint32_t n_more, uint64_t max_samples = 0, const uint64_t* new_stream = nullptr) {
        if (!prm_) return base::PlanningError::PlannerUninitialised;
        oxhip_prm_grow_config g{};
        g.struct_size = sizeof g;
        g.n_more = n_more;
        g.max_samples = max_samples;
        if (new_stream) { g.flags = OXHIP_PRM_GROW_NEW_STREAM; g.stream = *new_stream; }
        Growth out;
        grow_status_ = oxhip_prm_grow_roadmap(prm_, &g, &out.added, &out.samples_drawn);
        if (grow_status_ != OXHIP_OK) return to_error(grow_status_);
        return out;
    }
    int32_t last_grow_status() const { return grow_status_; }
    // The roadmap's connected components (oxhip_prm_components): label[i] = the lowest milestone index of i's component,
    // size[i] = its milestones; the largest component's ties go to the lowest label.  Only the graph is read.
    struct Components {
        std::vector<uint32_t> label, size;
        uint32_t n_components = 0, largest_label = 0, largest_size = 0;
    };
    Result<Components, base::PlanningError> components() {
        if (!prm_) return base::PlanningError::PlannerUninitialised;
        Components out;
        const uint32_t n = (uint32_t)num_milestones();
        out.label.assign(n, 0);
        out.size.assign(n, 0);
        const int32_t st = oxhip_prm_components(prm_, n ? out.label.data() : nullptr, n ? out.size.data() : nullptr, n, &out.n_components,
                                                &out.largest_label, &out.largest_size);
        if (st != OXHIP_OK) return to_error(st);
        return out;
    }
    // Removes milestones and renumbers the rest in their old order (oxhip_prm_prune).  `flags` = OXHIP_PRM_PRUNE_INVALID |
    // _MASK | _MIN_SIZE | _LARGEST; `keep` (one byte per milestone) iff _MASK.  A refused argument or a call that would keep no
    // milestone (OXHIP_ERR_BAD_ARG, kept in last_prune_status(), the text in oxhip_last_error_string()) comes back as
    // NoSolutionFound and leaves the roadmap as it was.
    struct Pruning {
        std::vector<int32_t> new_index;   // [milestones before] -1 = dropped
        uint32_t kept = 0;
        uint64_t removed_entries = 0;
    };
    Result<Pruning, base::PlanningError> prune(uint32_t flags, uint32_t min_size = 0, const std::vector<uint8_t>* keep = nullptr) {
        if (!prm_) return base::PlanningError::PlannerUninitialised;
        oxhip_prm_prune_config c{};
        c.struct_size = sizeof c;
        c.flags = flags;
        c.min_size = min_size;
        Pruning out;
        const size_t n = num_milestones();
        if (keep && keep->size() != n) { prune_status_ = OXHIP_ERR_BAD_ARG; return to_error(prune_status_); }
        out.new_index.assign(n, -1);
        prune_status_ = oxhip_prm_prune(prm_, &c, keep ? keep->data() : nullptr, n ? out.new_index.data() : nullptr, &out.kept,
                                        &out.removed_entries);
        if (prune_status_ != OXHIP_OK) return to_error(prune_status_);
        return out;
    }
    int32_t last_prune_status() const { return prune_status_; }
    int32_t last_status() const { return last_status_; }

  private:
    static base::PlanningError to_error(int32_t st) {
        switch (st) {
            case OXHIP_ERR_TIMEOUT: return base::PlanningError::Timeout;
            case OXHIP_ERR_PLANNER_UNINITIALISED: return base::PlanningError::PlannerUninitialised;
            case OXHIP_ERR_INVALID_START_STATE: return base::PlanningError::InvalidStartState;
            case OXHIP_ERR_UNSAMPLED_STATE_SPACE: return base::PlanningError::UnsampledStateSpace;
            default: return base::PlanningError::NoSolutionFound;
        }
    }
    void reset() {
        if (prm_) (void)oxhip_prm_destroy(prm_);
        prm_ = nullptr;
    }
    oxhip_prm* prm_ = nullptr;
    std::size_t last_batch_ = 0;   // problems of the last solve_batch / solve_batch_shortest
    std::shared_ptr<base::ProblemDefinition> pd_;
    int32_t last_status_ = OXHIP_ERR_PLANNER_UNINITIALISED;
    int32_t set_roadmap_status_ = OXHIP_OK;
    int32_t simplify_status_ = OXHIP_OK;
    int32_t grow_status_ = OXHIP_OK;
    int32_t prune_status_ = OXHIP_OK;
};

}  // namespace geometric
}  // namespace oxmpl
