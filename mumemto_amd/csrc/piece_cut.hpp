// piece_cut.hpp -- where a text of whole lines is cut into pieces (text_pieces.hpp).  Plain C++: a host compiler alone
// builds it (tests/piece_cut_check.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mmt {

struct PieceCuts {
    std::vector<size_t> cut;      // ascending from 0 to n: piece i holds the lines [cut[i], cut[i + 1])
    uint64_t longest = 0;         // bytes of the longest piece
};

// off: n + 1 ascending byte offsets, line r is [off[r], off[r + 1]).  A piece takes as many whole lines as piece_bytes hold;
// a line longer than that is a piece of its own.
inline PieceCuts cut_pieces(const uint64_t* off, size_t n, uint64_t piece_bytes) {
    PieceCuts c;
    c.cut.push_back(0);
    for (size_t r = 0; r < n;) {
        const uint64_t lim = off[r] + piece_bytes;
        size_t q = (size_t)(std::upper_bound(off + r + 1, off + n + 1, lim) - off) - 1;
        if (q <= r) q = r + 1;
        c.longest = std::max<uint64_t>(c.longest, off[q] - off[r]);
        c.cut.push_back(q);
        r = q;
    }
    return c;
}

}  // namespace mmt
