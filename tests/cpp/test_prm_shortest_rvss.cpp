// PRM::solve_batch_shortest of include/oxmpl/oxmpl.hpp on the scene of test_prm_batch_rvss.cpp: the outcomes are solve_batch's,
// problem by problem; a solved problem's path starts at the start state, ends inside the goal ball and is no longer than the
// breadth-first one.  Exit code 0 = all assertions hold; 77 = no GPU (the planner refuses to run: no CPU fallback).
#include <cmath>
#include <cstdio>
#include <cstring>
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

static double dist(const RealVectorState& a, const RealVectorState& b) {
    return std::sqrt((a.values[0] - b.values[0]) * (a.values[0] - b.values[0]) + (a.values[1] - b.values[1]) * (a.values[1] - b.values[1]));
}

static double length(const Path& p) {
    double c = 0.0;
    for (std::size_t k = 1; k < p.states.size(); ++k) c += dist(p.states[k - 1], p.states[k]);
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
    for (auto& r : planner.solve_batch_shortest(problems, std::chrono::seconds(5)))
        CHECK(r.is_err() && r.err() == PlanningError::PlannerUninitialised, "solve_batch_shortest before setup");
    planner.setup(problems[0], checker);
    if (oxhip_device_count(&ndev) != OXHIP_OK) {
        CHECK(planner.last_status() == OXHIP_ERR_NO_DEVICE, "without a GPU setup must fail loudly");
        for (auto& r : planner.solve_batch_shortest(problems, std::chrono::seconds(5))) CHECK(r.is_err(), "no CPU fallback");
        std::printf("no GPU: refused as designed\n");
        return 77;
    }
    CHECK(planner.last_status() == OXHIP_OK, "setup");
    for (auto& r : planner.solve_batch_shortest(problems, std::chrono::seconds(5)))
        CHECK(r.is_err() && r.err() == PlanningError::UnsampledStateSpace, "solve_batch_shortest before construct_roadmap");
    CHECK(planner.construct_roadmap().is_ok(), "Issue constructing roadmap!");
    auto bfs = planner.solve_batch(problems, std::chrono::seconds(5));
    auto batch = planner.solve_batch_shortest(problems, std::chrono::seconds(5));
    CHECK(batch.size() == problems.size(), "one result per problem");
    CHECK(planner.solve_batch_shortest({}, std::chrono::seconds(5)).empty(), "an empty batch");
    CHECK(batch[0].is_ok() && batch[3].is_ok(), "solvable problems are solved");
    CHECK(batch[1].is_err() && batch[1].err() == PlanningError::InvalidStartState, "start inside the wall");
    CHECK(batch[2].is_err() && batch[2].err() == PlanningError::NoSolutionFound, "goal outside the bounds");
    for (std::size_t i = 0; i < problems.size(); ++i) {
        CHECK(bfs[i].is_ok() == batch[i].is_ok(), "same outcome as solve_batch");
        if (bfs[i].is_err()) {
            CHECK(bfs[i].err() == batch[i].err(), "same error");
            continue;
        }
        const Path &a = bfs[i].unwrap(), &b = batch[i].unwrap();
        CHECK(b.states.size() >= 2, "a path has the start state and a milestone");
        CHECK(std::memcmp(b.states[0].values.data(), problems[i]->start_states[0].values.data(), 2 * sizeof(double)) == 0, "starts at the start");
        CHECK(dist(b.states.back(), problems[i]->goal->target()) <= problems[i]->goal->radius(), "ends inside the goal ball");
        CHECK(length(b) <= length(a) * (1.0 + 1e-12), "no longer than the breadth-first path");
        CHECK(b.states.size() >= a.states.size(), "the breadth-first path has the fewest states");
    }
    std::printf("PRM shortest batch test passed!\n");
    return 0;
}
