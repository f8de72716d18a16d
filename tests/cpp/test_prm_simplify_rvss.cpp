// PRM::simplify_batch, PRM::is_valid and PRM::check_motion of include/oxmpl/oxmpl.hpp on the scene of test_prm_batch_rvss.cpp: a
// simplified path keeps both ends of its raw path, every link of it passes the planner's own check_motion and it is no longer;
// a refused solve_batch leaves the last batch, and so what simplify_batch returns, as they were.
// Exit code 0 = all assertions hold; 77 = no GPU (the planner refuses to run: no CPU fallback).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>

#include "oxmpl/oxmpl.hpp"

using namespace oxmpl::base;
using oxmpl::geometric::PRM;

struct WallObstacleChecker : StateValidityChecker {
    std::vector<Box> boxes() const override { return {Box{{4.75, 2.0}, {5.25, 8.0}}}; }
};

struct CircularGoalRegion : GoalSampleableRegion {
    RealVectorState target_;
    double radius_;
    CircularGoalRegion(RealVectorState t, double r) : target_(std::move(t)), radius_(r) {}
    RealVectorState target() const override { return target_; }
    double radius() const override { return radius_; }
};

#define CHECK(cond, msg) do { if (!(cond)) { std::printf("FAILED: %s\n", msg); return 1; } } while (0)

static double length(const Path& p) {
    double c = 0.0;
    for (std::size_t k = 1; k < p.states.size(); ++k)
        c += std::hypot(p.states[k].values[0] - p.states[k - 1].values[0], p.states[k].values[1] - p.states[k - 1].values[1]);
    return c;
}

int main() {
    int32_t ndev = 0;
    std::vector<std::pair<double, double>> bounds{{0.0, 10.0}, {0.0, 10.0}};
    auto space = std::make_shared<RealVectorStateSpace>(RealVectorStateSpace::create(2, &bounds).unwrap());
    auto problem = [&](double sx, double sy, double gx, double gy, double r) {
        return std::make_shared<ProblemDefinition>(
            ProblemDefinition{space, {RealVectorState({sx, sy})}, std::make_shared<CircularGoalRegion>(RealVectorState({gx, gy}), r)});
    };
    std::vector<std::shared_ptr<ProblemDefinition>> problems{problem(1.0, 5.0, 9.0, 5.0, 0.5), problem(5.0, 5.0, 9.0, 5.0, 0.5),
                                                             problem(1.0, 5.0, 20.0, 20.0, 0.5), problem(9.0, 9.0, 1.0, 1.0, 0.4)};
    auto checker = std::make_shared<WallObstacleChecker>();
    PRM planner(5.0, 0.5);
    CHECK(planner.simplify_batch().empty() && planner.last_simplify_status() == OXHIP_ERR_PLANNER_UNINITIALISED, "simplify_batch before setup");
    CHECK(!planner.is_valid(RealVectorState({1.0, 5.0})), "is_valid before setup");
    planner.setup(problems[0], checker);
    if (oxhip_device_count(&ndev) != OXHIP_OK) {
        CHECK(planner.last_status() == OXHIP_ERR_NO_DEVICE, "without a GPU setup must fail loudly");
        CHECK(planner.simplify_batch().empty() && planner.last_simplify_status() != OXHIP_OK, "no CPU fallback");
        std::printf("no GPU: refused as designed\n");
        return 77;
    }
    CHECK(planner.last_status() == OXHIP_OK, "setup");
    CHECK(planner.is_valid(RealVectorState({1.0, 5.0})) && !planner.is_valid(RealVectorState({5.0, 5.0})), "is_valid");
    CHECK(planner.check_motion(RealVectorState({1.0, 5.0}), RealVectorState({4.0, 5.0})), "a free motion");
    CHECK(!planner.check_motion(RealVectorState({1.0, 5.0}), RealVectorState({9.0, 5.0})), "a motion through the wall");
    CHECK(planner.construct_roadmap().is_ok(), "Issue constructing roadmap!");
    CHECK(planner.simplify_batch().empty() && planner.last_simplify_status() == OXHIP_ERR_UNSAMPLED_STATE_SPACE, "no batch yet");
    auto raw = planner.solve_batch_shortest(problems, std::chrono::seconds(5));
    CHECK(raw.size() == 4 && raw[0].is_ok() && raw[3].is_ok() && raw[1].is_err() && raw[2].is_err(), "the batch");

    auto check = [&](const std::vector<oxmpl::Result<Path, PlanningError>>& simp) {
        if (simp.size() != raw.size()) return false;
        for (std::size_t i = 0; i < raw.size(); ++i) {
            if (raw[i].is_err()) {
                if (!simp[i].is_err() || !(simp[i].err() == raw[i].err())) return false;
                continue;
            }
            if (!simp[i].is_ok()) return false;
            const Path &a = raw[i].unwrap(), &b = simp[i].unwrap();
            if (b.states.size() < 2 || b.states.size() > (a.states.size() - 1) * 4 + 1) return false;
            if (std::memcmp(b.states.front().values.data(), a.states.front().values.data(), 2 * sizeof(double)) != 0) return false;
            if (std::memcmp(b.states.back().values.data(), a.states.back().values.data(), 2 * sizeof(double)) != 0) return false;
            for (std::size_t k = 1; k < b.states.size(); ++k)
                if (!planner.check_motion(b.states[k - 1], b.states[k])) return false;
            if (!(length(b) <= length(a) * (1.0 + 1e-12))) return false;
        }
        return true;
    };
    CHECK(check(planner.simplify_batch(4)) && planner.last_simplify_status() == OXHIP_OK, "simplify_batch(4)");
    CHECK(length(planner.simplify_batch(4)[0].unwrap()) < length(raw[0].unwrap()), "the path round the wall gets shorter");

    // a refused simplify: every entry carries the error, the planner stays usable
    auto refused = planner.simplify_batch(0);
    CHECK(refused.size() == 4 && refused[0].is_err() && planner.last_simplify_status() == OXHIP_ERR_BAD_ARG, "subdivide 0 is refused");
    CHECK(planner.last_status() == OXHIP_OK, "a refused simplify is not the planner's error");

    // a refused solve_batch -- by the library (a NaN start), by the wrapper (a state of another dimension) -- leaves the last
    // batch as it was: simplify_batch still answers for its four problems
    const double nan = std::numeric_limits<double>::quiet_NaN();
    auto bad = planner.solve_batch({problem(nan, 5.0, 9.0, 5.0, 0.5)}, std::chrono::seconds(5));
    CHECK(bad.size() == 1 && bad[0].is_err(), "a NaN start is refused");
    CHECK(check(planner.simplify_batch(4)), "simplify_batch after a batch the library refused");
    auto other = std::make_shared<ProblemDefinition>(
        ProblemDefinition{space, {RealVectorState({1.0, 5.0, 0.0})}, std::make_shared<CircularGoalRegion>(RealVectorState({9.0, 5.0}), 0.5)});
    auto bad2 = planner.solve_batch({other, other}, std::chrono::seconds(5));
    CHECK(bad2.size() == 2 && bad2[0].is_err(), "a state of another dimension is refused");
    CHECK(check(planner.simplify_batch(4)), "simplify_batch after a batch the wrapper refused");

    // a new, smaller batch replaces it
    auto one = planner.solve_batch({problems[3]}, std::chrono::seconds(5));
    CHECK(one.size() == 1 && one[0].is_ok(), "a batch of one");
    auto simp1 = planner.simplify_batch(2, 1);
    CHECK(simp1.size() == 1 && simp1[0].is_ok(), "simplify_batch follows the new batch's size");
    CHECK(planner.solve_batch({}, std::chrono::seconds(5)).empty() && planner.simplify_batch().empty()
              && planner.last_simplify_status() == OXHIP_OK, "an empty batch");
    std::printf("PRM simplify batch test passed!\n");
    return 0;
}
