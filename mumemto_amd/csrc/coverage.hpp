// coverage.hpp -- multi-MUM coverage of the sequences on the device (the reference's `mumemto coverage`:
// mumemto/mum_coverage.py:55-82, one sequence and one bitmap per invocation).
#pragma once
#include <cstdint>

#include "engine.hpp"
#include "merge_types.hpp"

namespace mmt {

struct CoverageStats {
    // HIP-event milliseconds: extraction, column sorts, running maximum + sum, runs
    float ms[4] = {0, 0, 0, 0};
    uint64_t cols_sorted = 0, cols_ascending = 0, batches = 0, runs = 0;
};

// For column c (seq_idx, or every column with seq_idx == -1) the union of the intervals [start, min(start + length,
// seq_lengths[c])) of the rows with start != -1 and length >= min_length: its size (m.cov_covered[c]) and its maximal
// stretches, the runs, half-open and ascending (m.d_runs, run r of column c at m.cov_run_begin[c] + r).  Intervals that touch
// belong to one run; strands play no part.  A pure reader of the table: rows, blocks and calls of m stay, partial rows are
// legal.  seq_lengths: n_docs host entries.  Throws std::invalid_argument for a null seq_lengths, a seq_idx outside
// [-1, n_docs) and a needed length <= 0; fewer than 2^32 rows, starts below 2^62.
void coverage(Engine& e, MergedRows& m, const int64_t* seq_lengths, int64_t seq_idx, int64_t min_length,
              CoverageStats* stats = nullptr);

}  // namespace mmt
