// bed.hpp -- BED intervals of collinear blocks and multi-MUMs in contig coordinates, on the device (the reference's
// `mumemto bed`: mumemto/mum_to_bed.py, one sequence and one pass over the text file per invocation).
#pragma once
#include <cstdint>
#include <string>

#include "engine.hpp"
#include "merge_types.hpp"

namespace mmt {

struct BedStats {
    // HIP-event milliseconds: select, gather, contig lookup, text (the text of every bed_text / bed_write_text since)
    float ms[4] = {0, 0, 0, 0};
    uint64_t records = 0, clamped = 0, batches = 0, text_bytes = 0;
};

// For column c (seq_idx, or every column with seq_idx == -1) the records of the table in ascending order of their first row.
// With blocks attached: one per block and one per row in no block with length >= min_single; without: one per row with a
// start in c and length >= min_single.  A block gives [start[first], start[last] + length[last]) when its last row is on '+'
// in c and [start[last], start[first] + length[first]) otherwise; a row gives [start, start + length).  The contig of a record
// is the first one whose cumulative length exceeds the interval's begin (contigs of length 0 are never chosen; a begin at or
// beyond the total gets the last contig and is counted in stats.clamped); the interval is not split at a contig's end.
// m.d_bed_records: 5 x int64 per record (contig within the column, rel_start, rel_end, name, strand), name = the block, or
// -1 - i for a row, i = its rank among the rows with a start in c; record k of column c at m.bed_record_begin[c] + k.
// Contigs of column c: contig_len / name_begin entries [contig_begin[c], contig_begin[c + 1]); name_begin has one more entry
// than there are contigs and indexes the byte blob names.  A pure reader of the table: rows, blocks, calls and coverage stay.
// Throws std::invalid_argument for a null table, a seq_idx outside [-1, n_docs), a needed column without contigs, with a
// negative contig length or of total length 0, and a needed name with a tab or a newline; fewer than 2^32 rows.
void bed(Engine& e, MergedRows& m, const uint64_t* contig_begin, const int64_t* contig_len, const uint64_t* name_begin,
         const char* names, int64_t seq_idx, int64_t min_single, BedStats* stats = nullptr);

// the lines of column col of the last bed(): `contig <TAB> rel_start <TAB> rel_end <TAB> block_<b> | mum_<i> <TAB> + | -`
std::string bed_text(Engine& e, const MergedRows& m, int64_t col, BedStats* stats = nullptr);
// the same bytes to a file, formatted and written in pieces (PieceWriter): PATH.tmp, renamed when complete
void bed_write_text(Engine& e, const MergedRows& m, int64_t col, const std::string& path, BedStats* stats = nullptr);

}  // namespace mmt
