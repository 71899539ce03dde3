// sequences.hpp -- the bases of the multi-MUMs of one column of a table as a multi-FASTA, on the device (the reference's
// src/extract_mums.cpp, which the string-based merge runs per partition, and its user tool mumemto/extract_mums.py).
#pragma once
#include <cstdint>
#include <string>

#include "engine.hpp"
#include "merge_types.hpp"

namespace mmt {

// The two forms of the reference differ in exactly these points:
//                                            BINARY (src/extract_mums.cpp)         PYTHON (mumemto/extract_mums.py)
//   bytes of a record                        as they are, not upper-cased          bases upper-cased (a-z)
//   strands                                  ignored: always the forward slice     rows on '-' are reverse-complemented
//   record separator                         every record ends in \n               joined by \n, none behind the last one
//   row that runs over the document's end    cut there                             cut there
//   row that starts exactly at the end       empty record                          empty record
//   row that starts beyond the end           refused                               empty record
//   row with no start in the column (-1)     refused (the binary's exit 1 on       empty record: what Python's slice
//                                            partial MUMs)                         [-1 : -1 + len] yields for any length up to
//                                                                                  the document's; that case is the rule here
// The complement table (A<->T, C<->G, M<->K, R<->Y, V<->B, H<->D, everything else unchanged) is decided in
// sequence_kernels.hip: the reference takes it from Biopython.
enum class SeqDialect : int { BINARY = 0, PYTHON = 1 };

// Where the bases come from.  resident: the engine's own text after a run (Engine::text_ref(), byte or packed layout);
// document c's forward strand begins at its doc_start.  That text is always upper case (build_text upper-cases it), so there
// BINARY gives upper case too.  Otherwise: `n` bases of ONE document on the host, uploaded one byte per base.
struct SeqSource {
    bool resident = true;
    const uint8_t* bases = nullptr;
    uint64_t n = 0;
};

struct SequencesStats {
    float ms[2] = {0, 0};       // HIP-event milliseconds: measure + prefix sum, format (of every text since the last sequences())
    uint64_t records = 0, bases = 0, clipped = 0, empty = 0, text_bytes = 0, pieces = 0;
};

// Record i of the text is `>mum_<i>\n`, the bases of row i in column col, `#` with terminator, and the separator; i is the
// row's index in table order.  Judges every row, measures every record and keeps the 64-bit record offsets with the table
// (m.d_seq_offset, n_rows + 1 entries).  A pure reader of the table: rows, blocks, calls, coverage, BED records and labels
// stay.  Throws std::invalid_argument, with nothing attached (sequences of an earlier call included), for: col outside
// [0, n_docs); a start below -1; 2^32 rows or more; null bases for a document of n > 0; a resident source when the engine
// holds no text or the table's column count is not the engine's n_docs(); and the dialect's refusals above, naming the first
// such row.
void sequences(Engine& e, MergedRows& m, const SeqSource& source, int64_t col, SeqDialect dialect, bool terminator,
               SequencesStats* stats = nullptr);
// the same with the document read from a FASTA file (mmt::read_fasta: plain or gzip, records concatenated); *doc_len = its bases
void sequences_file(Engine& e, MergedRows& m, const std::string& fasta, int64_t col, SeqDialect dialect, bool terminator,
                    SequencesStats* stats = nullptr, uint64_t* doc_len = nullptr);

// the text of the last sequences(); after a resident one, throws std::runtime_error once the engine has laid out a text again
// (Engine::text_generation(): any run, any text or stream handed over) -- the source positions are then measured anew
std::string sequences_text(Engine& e, const MergedRows& m, SequencesStats* stats = nullptr);
// the same bytes to a file, formatted and written in pieces of whole records (PieceWriter): PATH.tmp, renamed when complete
void sequences_write_text(Engine& e, const MergedRows& m, const std::string& path, SequencesStats* stats = nullptr);

}  // namespace mmt
