// inversion.hpp -- inversion calls from the collinear blocks of a row table on the device (the reference's
// `mumemto inversion`: mumemto/find_inversions.py main, find_reversals, inversion_coords).
#pragma once
#include <cstdint>

#include "engine.hpp"
#include "merge_types.hpp"

namespace mmt {

struct InversionStats {
    float ms[3] = {0, 0, 0};           // HIP-event milliseconds: gather of the block heads, column sorts, run passes
    uint64_t blocks = 0, cols_sorted = 0, cols_ascending = 0, runs = 0, calls = 0;
};

// A block list read from a file (n_blocks x (first row, last row), host memory) becomes the blocks of m, as if
// collinear_blocks() had found them.  Refused (std::invalid_argument): a block out of range, first > last, blocks not
// ascending and disjoint; a table with a partial row; column 0 not ascending.
void set_blocks(Engine& e, MergedRows& m, const uint32_t* lr, uint64_t n_blocks);

// For every column i >= 1: the blocks in ascending order of the start of their first row in i (ties by block number); every
// maximal stretch of that order in which the block number falls by one from position to position, at least two blocks, all of
// them on '-' in i, is a call (i, start, end, ref_start, ref_end): start = starts[last row of the first block, i], end =
// starts[first row of the last block, i] + its length, the same two rows in column 0 for the reference.  max_length >= 0
// keeps |end - start| <= max_length only.  Calls are in ascending order of (i, position); they go to m.d_calls.
void inversion_calls(Engine& e, MergedRows& m, int64_t max_length, InversionStats* stats = nullptr);

}  // namespace mmt
