// The shortcut's host rules (oxmpl_amd/csrc/oxhip_host.hpp: shortcut_shape, shortcut_rounds, shortcut_matrix_bytes): pure host
// arithmetic, built with -fsanitize=address,undefined and run on the CPU.  The program reads one case per line and prints what the
// helpers give; tests/test_shortcut_host.py writes the cases and compares with the Python models.
//   shape L m max_span                                   -> shape rows window words checks
//   rounds m max_span budget_bytes max_paths n len...    -> rounds ok | q0 w0 w1 .. | q0 ..   (every round: its first path and the prefix
//                                                           sums of its paths' words)   or   rounds refused q
//   matrix L m max_span n_words word(hex)...             -> matrix M row row ..   (each row M characters 0 / 1)
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../oxmpl_amd/csrc/oxhip_host.hpp"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind;
        in >> kind;
        if (kind == "shape") {
            uint32_t L, m, span;
            in >> L >> m >> span;
            const oxhip::ShortcutShape s = oxhip::shortcut_shape(L, m, span);
            std::printf("shape %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", s.rows, s.window, s.words, s.checks);
        } else if (kind == "rounds") {
            uint32_t m, span, max_paths, n;
            uint64_t budget;
            in >> m >> span >> budget >> max_paths >> n;
            std::vector<uint32_t> len(n), first{77u};   // (what `first` held before is dropped)
            for (uint32_t& l : len) in >> l;
            uint32_t refused = 0xFFFFFFFFu;
            if (!oxhip::shortcut_rounds(len.data(), n, m, span, budget, max_paths, first, refused)) {
                std::printf("rounds refused %u\n", refused);
                continue;
            }
            std::printf("rounds ok");
            for (size_t r = 0; r + 1 < first.size(); ++r) {
                uint64_t w = 0;
                std::printf(" | %u %" PRIu64, first[r], w);
                for (uint32_t q = first[r]; q < first[r + 1]; ++q) std::printf(" %" PRIu64, w += oxhip::shortcut_shape(len[q], m, span).words);
            }
            std::printf(" | end %u\n", first.empty() ? 0u : first.back());
        } else if (kind == "matrix") {
            uint32_t L, m, span;
            size_t n_words;
            in >> L >> m >> span >> n_words;
            std::vector<uint64_t> bits(n_words);   // exactly the matrix's words: a read past them is the sanitizer's to report
            for (uint64_t& w : bits) in >> std::hex >> w;
            const uint64_t M = oxhip::shortcut_shape(L, m, span).rows;
            std::vector<uint8_t> out(M * M, 7);
            oxhip::shortcut_matrix_bytes(bits.data(), L, m, span, out.data());
            std::printf("matrix %" PRIu64, M);
            for (uint64_t u = 0; u < M; ++u) {
                std::printf(" ");
                for (uint64_t v = 0; v < M; ++v) std::printf("%u", (unsigned)out[u * M + v]);
            }
            std::printf("\n");
        } else if (!kind.empty()) {
            std::printf("unknown case %s\n", kind.c_str());
            return 1;
        }
    }
    std::printf("shortcut host rules: done\n");
    return 0;
}
