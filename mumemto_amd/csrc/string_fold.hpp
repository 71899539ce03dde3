// string_fold.hpp -- the last step of the string-based merge on the device (the reference's mumemto/merge_mums.py:211-307): the
// MUMs of the partitions' MUM strings mapped back through the partitions' rows, and the partitions' threshold tables merged
// position by position.  The closed form is mumemto_amd/merge_mums.py string_merge; this restates it and changes nothing of it.
#pragma once
#include <cstdint>

#include "engine.hpp"
#include "merge_types.hpp"

namespace mmt {

struct StringFoldStats {
    // HIP-event milliseconds: split, locate and test, assemble + sort + permute, thresholds
    float ms[4] = {0, 0, 0, 0};
    uint64_t pieces = 0, dropped_short = 0, dropped_thresh = 0, rows = 0;
};

// parts[0 .. S): the partitions' rows, in ascending order of their first column, and their threshold tables; mom: the rows of the
// MUMs of MUMs (its threshold fields are not read); records: per collection the record lengths of mom's .lengths file.  All
// host arrays.  The result carries the merged rows over all the partitions' columns, in ascending (stable) order of column 0,
// and the merged thresh / thresh_rev (d_string_thresh, d_string_thresh_rev: the rows' positions, a 0 behind every row).
// Throws std::invalid_argument, before anything is launched over the table at fault, for: a number of partitions that is not
// mom's number of columns or the number of collections ("input # of MUM files does not match merged MUM input file"); 2^32 - 1
// rows or more in a table, or 2^32 - 256 pieces; a partition without columns; a negative record length; more records in a collection than
// its partition has rows; an absent start (-1) anywhere; a partition whose first column is not ascending; a threshold table
// whose length is not the sum of length + 1 over the partition's rows.
MergedRows string_fold(Engine& e, const mmt_string_part* parts, size_t S, const mmt_string_part* mom, const mmt_string_records* records,
                       StringFoldStats* stats = nullptr);

}  // namespace mmt
