// label.hpp -- every start of the table as (contig, offset inside that contig), and the six-field text of it, on the device
// (the reference's `mumemto label`: mumemto/get_sequence_info.py).
#pragma once
#include <cstdint>
#include <string>

#include "engine.hpp"
#include "merge_types.hpp"

namespace mmt {

struct LabelStats {
    // HIP-event milliseconds: lookup, measure + prefix sum, write, device-to-host copies (+ the host's wait for the file);
    // of the last label() and of every label_text / label_write_text since
    float ms[4] = {0, 0, 0, 0};
    uint64_t cells = 0, absent = 0, hbm_columns = 0, text_bytes = 0;
};

// Cell (r, c) with start s: the contig is the first k of column c with ends_k > s (ends_k = len_0 + ... + len_k; a contig of
// length 0 is never chosen), the offset s - (ends_k - len_k); s == -1 gives contig 0 and offset -1.  m.d_label_contig (u32)
// and m.d_label_rel (i64) hold them row-major like the table.  Contigs of column c: contig_len / name_begin entries
// [contig_begin[c], contig_begin[c + 1]); names and name_begin are read with use_names only.  stats->text_bytes receives the
// length of the text with the blocks attached now.  A pure reader of the table: rows, blocks, calls, coverage and BED records
// stay.  Throws std::invalid_argument for null tables, a column without contigs, with a negative contig length or of total
// length 0, with use_names a name with a tab, a newline or a comma, and for a start at or beyond its sequence's total (the
// first such cell in row-major order is named); fewer than 2^32 rows.  A call that throws leaves no labels attached, those of an
// earlier call included.
void label(Engine& e, MergedRows& m, const uint64_t* contig_begin, const int64_t* contig_len, const uint64_t* name_begin,
           const char* names, bool use_names, LabelStats* stats = nullptr);

// one line per row, in row order: LEN \t starts \t strands \t BLOCK \t contigs \t offsets \n, absent cells as -1; BLOCK is * for a
// table without blocks, else the row's block among those attached now, or -
std::string label_text(Engine& e, const MergedRows& m, LabelStats* stats = nullptr);
// the same bytes to a file, formatted and written in pieces of whole rows (PieceWriter): PATH.tmp, renamed when complete
void label_write_text(Engine& e, const MergedRows& m, const std::string& path, LabelStats* stats = nullptr);

}  // namespace mmt
