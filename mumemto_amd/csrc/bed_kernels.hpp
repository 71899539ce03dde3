// bed_kernels.hpp -- device side of the BED writer (the reference's `mumemto bed`: mumemto/mum_to_bed.py, a state machine
// over the rows of one column of the text file, a numpy searchsorted over the contig ends, one Python format per line).
//
// Here a record is selected per row (the head of a collinear block, or a free row that is long enough), numbered by a prefix
// sum, and names its two rows: first and last (the same row for a free one).  Per column the record's interval is gathered from
// those two rows, looked up among the cumulative contig lengths of the column, and kept as 5 x int64.  The text of a column is
// measured, summed and written from those records.
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

namespace mmt { namespace bk {

constexpr uint32_t SELECT_BLOCK = 256, SELECT_ITEMS = 4, SELECT_TILE = SELECT_BLOCK * SELECT_ITEMS;   // rows of one workgroup
constexpr uint32_t BED_LDS_CONTIGS = 1024;      // contig ends of a column a workgroup of the lookup stages in LDS (8 KB)
constexpr uint32_t BED_WAVE_RECORDS = 64;       // records of one wave of the writer: a line per lane
constexpr uint32_t BED_LDS_BYTES = 8192;        // the lines of a wave are staged in LDS when together they are no longer
constexpr uint32_t RECORD_FIELDS = 5;           // contig, rel_start, rel_end, name, strand
constexpr uint32_t NO_BLOCK = 0xffffffffu;

// flag[r] = row r makes a record.  With blocks (row_block, blocks non-null): the first row of its block, or in no block and
// length[r] >= min_single.  Without: a start other than -1 in column col and length[r] >= min_single; present[r] = the start
// is not -1 (present is not written with blocks).
void select_flags(const int64_t* off, const uint32_t* length, const uint32_t* row_block, const uint32_t* blocks, uint32_t n,
                  uint32_t n_docs, uint32_t col, int64_t min_single, uint32_t* flag, uint32_t* present, hipStream_t s);
// number[r] = exclusive sum of flag, rank[r] = exclusive sum of present (null with blocks).  Record k = number[r] of a flagged
// row: rows[2 k], rows[2 k + 1] = its first and last row, name[k] = the block, or -1 - rank (-1 - r with blocks).
void list_records(const uint32_t* flag, const uint32_t* number, const uint32_t* rank, const uint32_t* row_block,
                  const uint32_t* blocks, uint32_t n, uint32_t* rows, int64_t* name, hipStream_t s);

// Columns [c0, c0 + n_cols) of the records' two rows through a tile transpose in LDS: a record's cells of the batch are
// contiguous in its row and are read n_cols x 8 bytes at a time; per column 64 records are written at a time.  With the strand
// of the last row: '+': [start[first], start[last] + length[last]); '-': [start[last], start[first] + length[first]).
// begin, end: [n_cols][n_rec]; strand likewise, 1 = '+'.
void gather(const int64_t* off, const uint8_t* st, const uint32_t* length, const uint32_t* rows, uint32_t n_rec, uint32_t n_docs,
            uint32_t c0, uint32_t n_cols, int64_t* begin, int64_t* end, uint8_t* strand, hipStream_t s);

// Column c0 + j, record k: the first contig i of the column with ends[i] > begin (ends: cumulative contig lengths, those of
// column c at ends[contig_begin[c] .. contig_begin[c + 1])); none: the last contig, and *clamped += 1.  The record goes to
// records[(j * n_rec + k) * 5]: i, begin - (ends[i] - len_i), that + (end - begin), name[k], strand.  A workgroup stages the
// ends of its column in LDS when they are at most BED_LDS_CONTIGS and searches HBM otherwise.  Every column has a contig.
void lookup(const int64_t* begin, const int64_t* end, const uint8_t* strand, const int64_t* name, uint32_t n_rec, uint32_t c0,
            uint32_t n_cols, const uint64_t* contig_begin, const int64_t* ends, int64_t* records, uint64_t* clamped, hipStream_t s);

// bytes[k] = length of the line of record k: name of the contig (name_begin: offsets of the global contig first_contig + i
// into the blob), three decimals (rel_end may be negative), block_<b> or mum_<i>, four tabs, the strand, the newline
void measure(const int64_t* records, uint32_t n_rec, const uint64_t* name_begin, uint64_t first_contig, uint32_t* bytes,
             hipStream_t s);
// the lines of records [0, n_rec) at text + offset[k] - base; a wave takes BED_WAVE_RECORDS records: its lines are built in
// LDS and leave as one contiguous span in 8-byte stores (bytes up to the first aligned address and behind the last one on
// their own) when the span is at most BED_LDS_BYTES; longer spans are stored by every lane byte by byte
void write_lines(const int64_t* records, uint32_t n_rec, const uint64_t* name_begin, const char* names, uint64_t first_contig,
                 const uint64_t* offset, uint64_t base, char* text, hipStream_t s);

}}  // namespace mmt::bk
