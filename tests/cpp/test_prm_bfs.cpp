// prm_bfs_path (oxmpl_amd/csrc/oxhip_host.hpp): Planner::solve's graph search (prm.rs:266-304) and reconstruct_path on hand-made
// CSR roadmaps of 1 to 8 nodes.  Pure host code: built with -fsanitize=address,undefined and run on the CPU.  The expected chains
// follow the reference's FIFO by hand: the start connections enqueued twice, a node's neighbours in ascending order, the
// goal test at the pop.  (The oracle takes no roadmap from outside, it only samples its own; the GPU suites compare
// oxhip_prm_solve, which calls this function, with the oracle's paths on sampled roadmaps.)
#include <cstdio>
#include <limits>
#include <utility>
#include <vector>

#include "../../oxmpl_amd/csrc/oxhip_host.hpp"

using oxhip::PrmBfs;
typedef std::vector<uint32_t> U32;
static const double kNone = std::numeric_limits<double>::infinity();
static int failures = 0;

struct Graph {
    U32 offsets, nbrs;
    Graph(uint32_t n, const std::vector<std::pair<uint32_t, uint32_t>>& edges) {   // undirected edges -> CSR, every row ascending
        for (uint32_t u = 0; u < n; ++u) {
            offsets.push_back((uint32_t)nbrs.size());
            for (uint32_t v = 0; v < n; ++v)
                for (const auto& e : edges)
                    if ((e.first == u && e.second == v) || (e.second == u && e.first == v)) nbrs.push_back(v);
        }
        offsets.push_back((uint32_t)nbrs.size());
    }
};

// flags: bit 0 = start connection, bit 1 = goal milestone, as the query kernel writes them
static void expect(const char* name, const Graph& g, const U32& starts, const U32& goals, double timeout_s, PrmBfs want, const U32& want_chain) {
    std::vector<uint8_t> flags(g.offsets.size() - 1, 0);
    for (uint32_t s : starts) flags[s] |= 1;
    for (uint32_t t : goals) flags[t] |= 2;
    U32 chain = {99u};   // (the function clears it)
    const PrmBfs got = oxhip::prm_bfs_path(g.offsets, g.nbrs, flags, starts, timeout_s, chain);
    const bool ok = got == want && chain == want_chain;
    std::printf("%-44s %s\n", name, ok ? "ok" : "FAILED");
    if (!ok) {
        std::printf("  outcome %d (want %d), chain:", (int)got, (int)want);
        for (uint32_t c : chain) std::printf(" %u", c);
        std::printf("\n");
        ++failures;
    }
}

int main() {
    const Graph one(1, {}), line(3, {{0, 1}, {1, 2}}), diamond(4, {{0, 1}, {0, 2}, {1, 3}, {2, 3}}), two_parts(4, {{0, 1}, {2, 3}});
    const Graph eight(8, {{2, 3}, {5, 4}, {3, 7}, {4, 7}, {0, 1}, {1, 6}}), lonely(3, {{1, 2}});
    // the goal is a start connection: a chain of one (a path of start + 1 states)
    expect("goal is a start connection", one, {0}, {0}, kNone, PrmBfs::found, {0});
    expect("goal is the second start connection", line, {0, 2}, {2}, kNone, PrmBfs::found, {2});
    // two equally short routes: 0-1-3 and 0-2-3.  Node 0's row is (1, 2), so 1 is expanded first and claims 3
    expect("two equally short routes", diamond, {0}, {3}, kNone, PrmBfs::found, {3, 1, 0});
    // queue 2 5 2 5: 2 gives 3, 5 gives 4, 3 is popped before 4 and claims 7
    expect("two start connections, equal depth", eight, {2, 5}, {7}, kNone, PrmBfs::found, {7, 3, 2});
    expect("the nearer of two goals", eight, {0}, {6, 1}, kNone, PrmBfs::found, {1, 0});
    expect("goal in another component", two_parts, {0}, {3}, kNone, PrmBfs::unreachable, {});
    expect("goal in another component, 8 nodes", eight, {0}, {7}, kNone, PrmBfs::unreachable, {});
    expect("empty start set", line, {}, {2}, kNone, PrmBfs::empty_set, {});
    expect("empty goal set", line, {0}, {}, kNone, PrmBfs::empty_set, {});
    expect("isolated start connection", lonely, {0}, {2}, kNone, PrmBfs::unreachable, {});
    expect("isolated start connection beside a live one", lonely, {0, 1}, {2}, kNone, PrmBfs::found, {2, 1});
    // a zero timeout has passed at the first pop (prm.rs:285-287: elapsed > timeout), before the goal test
    expect("zero timeout, three pops needed", line, {0}, {2}, 0.0, PrmBfs::timed_out, {});
    expect("the same graph without a timeout", line, {0}, {2}, kNone, PrmBfs::found, {2, 1, 0});
    expect("a timeout that does not pass", line, {0}, {2}, 3600.0, PrmBfs::found, {2, 1, 0});
    if (failures) return 1;
    std::printf("prm_bfs_path: all cases passed\n");
    return 0;
}
