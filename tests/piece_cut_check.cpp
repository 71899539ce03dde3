// piece_cut_check.cpp -- cut_pieces (mumemto_amd/csrc/piece_cut.hpp) as a stand-alone program for the host sanitizers
// (tests/test_text_pieces_host.py builds and runs it).
//   piece_cut_check CASES    every line of CASES is "piece_bytes n off[0] ... off[n]"; prints "longest cut[0] cut[1] ..." per line
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "piece_cut.hpp"

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: piece_cut_check CASES\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        uint64_t piece = 0;
        size_t n = 0;
        if (!(ss >> piece >> n)) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
        std::vector<uint64_t> off(n + 1);                    // (exactly n + 1 entries: a read beyond them is the sanitizer's)
        for (auto& o : off)
            if (!(ss >> o)) { std::fprintf(stderr, "short case: %s\n", line.c_str()); return 2; }
        const mmt::PieceCuts c = mmt::cut_pieces(off.data(), n, piece);
        std::printf("%llu", (unsigned long long)c.longest);
        for (size_t q : c.cut) std::printf(" %zu", q);
        std::printf("\n");
    }
    return 0;
}
