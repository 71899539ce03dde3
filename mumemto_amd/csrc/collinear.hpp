// collinear.hpp -- collinear blocks of multi-MUMs on the device (the reference's `mumemto collinear`:
// mumemto/collinear_block.py:46-65 on top of mumemto/utils.py:9-64 find_coll_blocks).
#pragma once
#include <cstdint>

#include "engine.hpp"
#include "merge_types.hpp"

namespace mmt {

struct CollinearStats {
    // HIP-event milliseconds: filter + sort of the table, column extraction, column sorts, adjacency, blocks
    float ms[5] = {0, 0, 0, 0, 0};
    uint64_t rows_in = 0, rows_kept = 0, cols_sorted = 0, cols_ascending = 0, batches = 0, table_sorted = 0;
};

// The table of m becomes the one MUMdata holds when find_coll_blocks runs: partial rows (a -1 in any column) dropped, rows in
// ascending order of column 0 (stable).  Then every row gets its block (m.d_row_block) and the blocks their first and last
// rows (m.d_blocks); nothing of the table travels to the host.  max_break == 0: no gap limit; min_single < 0: no singleton
// blocks.  Equal starts in one column are ordered by row (the reference leaves that order to an unstable sort).
void collinear_blocks(Engine& e, MergedRows& m, uint32_t max_break, int64_t min_single, CollinearStats* stats = nullptr);

}  // namespace mmt
