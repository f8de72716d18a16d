// The RRT batch's filter thresholds (oxmpl_amd/csrc/oxhip_host.hpp: connect_grid_threshold, midpoint_threshold,
// star_edge_threshold, filter_maxabs): pure host arithmetic, built with -fsanitize=address,undefined and run on the CPU.  The
// program prints every input and result as a bit pattern; tests/test_rrt_filter_host.py restates the formulas and compares bit for
// bit, and checks that the thresholds are conservative with exact rationals.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../oxmpl_amd/csrc/oxhip_host.hpp"

static uint64_t bits(double v) {
    uint64_t u;
    std::memcpy(&u, &v, sizeof u);
    return u;
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const std::vector<double> radii = {-inf, -1e150, -2.5, -0.0, 0.0, 5e-324, 1e-9, 0.1, 0.75, 1.0, 3.0, 1234.5678, 1e150, inf, nan};
    const std::vector<double> hs = {1e-9, 0.25 * (1.0 + 1e-6) + 1e-9, 3.7, 1e3 + 1e-6};
    for (double r : radii) std::printf("connect %016" PRIx64 " %016" PRIx64 "\n", bits(r), bits(oxhip::connect_grid_threshold(r)));
    for (double r : radii)
        for (double h : hs) std::printf("midpoint %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", bits(r), bits(h), bits(oxhip::midpoint_threshold(r, h)));
    for (double r : radii)
        for (size_t i = 0; i < hs.size(); ++i)
            for (size_t j = i; j < hs.size(); ++j)
                std::printf("star %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", bits(r), bits(hs[i]), bits(hs[j]),
                            bits(oxhip::star_edge_threshold(r, hs[i], hs[j])));
    // the margin: bounds (2 * dim of them), centres, starts or none
    oxhip_rrt_config cfg{};
    cfg.dim = 3;
    const double bounds[8] = {-10.0, 10.0, -0.5, 0.25, -20.5, 3.0, 1e9, -1e9};   // (the last pair lies beyond dim: not read)
    for (int k = 0; k < 8; ++k) cfg.bounds[k] = bounds[k];
    const std::vector<double> none, centres = {1.0, -30.25, 2.0}, starts = {-4.0, 55.5, 0.0, 7.0, -8.0, 9.0};
    std::printf("maxabs bounds %016" PRIx64 "\n", bits(oxhip::filter_maxabs(cfg, none, nullptr)));
    std::printf("maxabs bounds+centres %016" PRIx64 "\n", bits(oxhip::filter_maxabs(cfg, centres, nullptr)));
    std::printf("maxabs bounds+centres+starts %016" PRIx64 "\n", bits(oxhip::filter_maxabs(cfg, centres, &starts)));
    std::printf("maxabs bounds+starts %016" PRIx64 "\n", bits(oxhip::filter_maxabs(cfg, none, &starts)));
    cfg.dim = 1;
    cfg.bounds[0] = -0.5; cfg.bounds[1] = 0.25;
    std::printf("maxabs small %016" PRIx64 "\n", bits(oxhip::filter_maxabs(cfg, none, &none)));   // never below 1
    std::printf("rrt filter thresholds: done\n");
    return 0;
}
