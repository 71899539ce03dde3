// label_kernels.hpp -- device side of the contig labels (the reference's `mumemto label`: mumemto/get_sequence_info.py, a numpy
// searchsorted per column over the cumulative contig lengths, then one Python join per row over six fields).
//
// Here every cell of the table finds its contig and its offset inside that contig in one pass (lookup); the outputs are
// row-major like the table, so that a row's line is formatted from three contiguous stretches.  The text is measured and
// written by a wave per row, as merge_kernels.hip does it for the .mums form, with three more fields.
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

#include "bed_kernels.hpp"

namespace mmt { namespace lk {

constexpr uint32_t LABEL_BLOCK = 256;           // work-items of a workgroup of the lookup
constexpr uint32_t LABEL_ROWS = 64;             // rows of one tile of the lookup
constexpr uint32_t LABEL_COLS = 32;             // columns of one batch: a workgroup stages the contig ends of these
constexpr uint32_t LABEL_LDS_UNITS = 4;         // staging units (bk::BED_LDS_CONTIGS ends each) of a workgroup: 32 KB of LDS
constexpr uint32_t LABEL_LDS_ENDS = LABEL_LDS_UNITS * bk::BED_LDS_CONTIGS;
constexpr uint32_t IN_HBM = 0xffffffffu;        // stage_at of a column whose ends are searched where they lie
constexpr uint64_t NO_CELL = ~0ull;             // *beyond when every start lies inside its sequence
constexpr uint32_t NO_BLOCK = 0xffffffffu;

// Rows [0, n) x columns [0, n_docs) of off (row-major): contig[r * n_docs + c] = the first k among the contigs of c with
// ends[k] > start (ends: cumulative contig lengths, those of column c at ends[contig_begin[c] .. contig_begin[c + 1])),
// rel[...] = start - (ends[k] - len_k); a start of -1 gives contig 0 and -1 and is counted in *absent.  A start at or beyond
// the last end of its column gives (0, -1) and reports (row0 + r) * n_docs + c through atomicMin on *beyond.  A workgroup
// owns the batch of LABEL_COLS columns blockIdx.y and walks tiles of LABEL_ROWS rows: consecutive work-items take consecutive
// cells of the batch's stretch of a row, for the read and for both writes.  stage_at[c]: where in the workgroup's LDS pool
// (LABEL_LDS_ENDS entries) the ends of column c are staged, IN_HBM: searched in HBM; chosen by the host (label.cpp).
void lookup(const int64_t* off, uint32_t n, uint32_t n_docs, uint64_t row0, const uint64_t* contig_begin, const int64_t* ends,
            const uint32_t* stage_at, uint32_t* contig, int64_t* rel, uint64_t* beyond, uint64_t* absent, hipStream_t s);

// bytes[r] = length of the line of row r:
//   LEN \t s_0,...  \t +,-,... \t BLOCK \t c_0,... \t rel_0,... \n
// with -1 printed for an absent start, BLOCK = `*` without block (null), else the row's block or `-`, and c_j the decimal contig
// or, with name_begin non-null, the name of contig contig_begin[j] + c_j (its length from name_begin).  A wave per row.
void measure(const uint32_t* len, const int64_t* off, const uint32_t* block, const uint32_t* contig, const int64_t* rel,
             uint32_t n, uint32_t n_docs, const uint64_t* contig_begin, const uint64_t* name_begin, uint64_t* bytes,
             hipStream_t s);
// the lines of rows [0, n) at text + text_off[r] - text_base, a wave per row.  The numeric fields: every lane formats a cell at
// the position a wave prefix sum of the widths gives it.  The names: the bytes of the field are dealt out to the lanes, 64 at
// a time, and every lane finds its byte's cell among the same prefix sums.
void write_lines(const uint32_t* len, const int64_t* off, const uint8_t* st, const uint32_t* block, const uint32_t* contig,
                 const int64_t* rel, uint32_t n, uint32_t n_docs, const uint64_t* contig_begin, const uint64_t* name_begin,
                 const char* names, const uint64_t* text_off, uint64_t text_base, char* text, hipStream_t s);

}}  // namespace mmt::lk
