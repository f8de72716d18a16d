// RRT::revalidate of include/oxmpl/oxmpl.hpp (oxhip_rrt_batch_revalidate_trees) on the scene of
// test_rrt_rvss.cpp: [0,10]^2, a wall x in [4.75,5.25], y in [2,8], start (1,5), circular goal (9,5) r=0.5.  The planner solves,
// a disc is dropped on the middle of its path, revalidate prunes the tree, and the next solve plans around the disc from what is
// left.  Exit code 0 = all assertions hold; 77 = no GPU (the planner refuses to run: no CPU fallback).
#include <cmath>
#include <cstdio>
#include <memory>

#include "oxmpl/oxmpl.hpp"

using namespace oxmpl::base;
using oxmpl::geometric::RRT;
using oxmpl::geometric::RRTConnect;
using oxmpl::geometric::RRTStar;

struct WallAndDiscs : StateValidityChecker {
    std::vector<Sphere> discs;
    std::vector<Box> boxes() const override { return {Box{{4.75, 2.0}, {5.25, 8.0}}}; }
    std::vector<Sphere> spheres() const override { return discs; }
};

struct CircularGoalRegion : GoalSampleableRegion {
    RealVectorState target_;
    double radius_;
    CircularGoalRegion(RealVectorState t, double r) : target_(std::move(t)), radius_(r) {}
    RealVectorState target() const override { return target_; }
    double radius() const override { return radius_; }
};

#define CHECK(cond, msg) do { if (!(cond)) { std::printf("FAILED: %s\n", msg); return 1; } } while (0)

int main() {
    int32_t ndev = 0;
    std::vector<std::pair<double, double>> bounds{{0.0, 10.0}, {0.0, 10.0}};
    auto space = std::make_shared<RealVectorStateSpace>(RealVectorStateSpace::create(2, &bounds).unwrap());
    RealVectorState start_state({1.0, 5.0});
    auto goal = std::make_shared<CircularGoalRegion>(RealVectorState({9.0, 5.0}), 0.5);
    auto pd = std::make_shared<ProblemDefinition>(ProblemDefinition{space, {start_state}, goal});
    auto wall = std::make_shared<WallAndDiscs>();

    RRT planner(0.5, 0.05);
    planner.seed = 3;
    CHECK(planner.revalidate().err() == PlanningError::PlannerUninitialised, "revalidate before setup");
    CHECK(oxhip_rrt_batch_revalidate_trees(nullptr, nullptr, nullptr) == OXHIP_ERR_BAD_ARG, "null batch");
    if (oxhip_device_count(&ndev) != OXHIP_OK) {
        planner.setup(pd, wall);
        CHECK(planner.last_status() == OXHIP_ERR_NO_DEVICE, "without a GPU setup must fail loudly");
        CHECK(planner.revalidate().is_err(), "no CPU fallback");
        std::printf("no GPU: refused as designed\n");
        return 77;
    }
    planner.setup(pd, wall);
    CHECK(planner.last_status() == OXHIP_OK, "setup");
    auto first = planner.solve(std::chrono::seconds(5));
    CHECK(first.is_ok(), "Planner failed to find a solution when one should exist.");
    const Path path = first.unwrap();
    const uint32_t n0 = planner.num_nodes();
    auto same = planner.revalidate();
    CHECK(same.is_ok() && same.unwrap() == 0, "unchanged obstacles remove nothing");
    CHECK(planner.num_nodes() == n0, "unchanged obstacles keep the tree");

    auto moved = std::make_shared<WallAndDiscs>();
    const RealVectorState& mid = path.states[path.states.size() / 2];
    moved->discs.push_back(Sphere{{mid.values[0], mid.values[1]}, 0.4});
    auto pruned = planner.revalidate(moved);
    CHECK(pruned.is_ok(), "revalidate");
    const uint32_t removed = pruned.unwrap();
    std::printf("%u of %u nodes removed\n", removed, n0);
    CHECK(removed > 0 && removed < n0 && planner.num_nodes() == n0 - removed, "a cut path loses nodes, not the tree");
    CHECK(!planner.is_valid(mid), "the new disc is in force");
    auto second = planner.solve(std::chrono::seconds(5));
    CHECK(second.is_ok(), "Planner failed to re-plan from the pruned tree.");
    for (auto& s : second.unwrap().states) CHECK(planner.is_valid(s), "the new path avoids the disc");
    CHECK(space->distance(second.unwrap().states.back(), goal->target()) <= goal->radius(), "Path should end in the goal region");

    RRTConnect pc(0.5, 0.0);
    pc.setup(pd, wall);
    CHECK(pc.revalidate().is_err(), "RRTConnect is refused");
    RRTStar ps(0.5, 0.0, 0.25);
    ps.setup(pd, wall);
    CHECK(ps.revalidate().is_err(), "RRTStar is refused");
    std::printf("RRT revalidate test passed!\n");
    return 0;
}
