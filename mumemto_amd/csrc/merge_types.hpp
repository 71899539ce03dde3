// merge_types.hpp -- result of the anchor merge (shared by engine.hpp and merge.hpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "device_utils.hpp"

namespace mmt {

// The merged rows live in HBM; host copies are made on demand (download_merged in merge.hpp).
struct MergedRows {
    size_t n_docs = 0, n_rows = 0, thresh_len = 0;
    DevBuf<uint32_t> d_length;
    DevBuf<int64_t> d_offsets;      // n_rows * n_docs, column 0 = anchor
    DevBuf<uint8_t> d_strands;      // 1 = '+'
    DevBuf<uint32_t> d_thresh;      // merged thresholds, L_0 + 1 entries, 32 bits (the 16-bit .athresh form: `thresh`, saturated)
    bool on_host = false;
    std::vector<uint32_t> length;
    std::vector<int64_t> offsets;
    std::vector<uint8_t> strands;
    std::vector<uint16_t> thresh;
    // collinear blocks (collinear.hpp), attached by collinear_blocks(): the table above is then the filtered, sorted one
    bool has_blocks = false;
    size_t n_blocks = 0;
    DevBuf<uint32_t> d_row_block;   // n_rows: block of the row, 0xFFFFFFFF = none
    DevBuf<uint32_t> d_blocks;      // n_blocks x (first row, last row)
    // inversion calls (inversion.hpp) over those blocks, attached by inversion_calls(); whatever replaces the blocks drops them
    bool has_calls = false;
    size_t n_calls = 0;
    DevBuf<int64_t> d_calls;        // n_calls x (column, start, end, ref_start, ref_end)
    // coverage (coverage.hpp), attached by coverage(): a reading of the table above; whatever replaces the table drops it
    bool has_coverage = false;
    std::vector<uint64_t> cov_covered;     // n_docs: covered positions of the column, 0 for a column not asked for
    std::vector<uint64_t> cov_run_begin;   // n_docs + 1: the runs of column c are [cov_run_begin[c], cov_run_begin[c + 1])
    DevBuf<uint64_t> d_run_begin;   // the same offsets in HBM
    DevBuf<int64_t> d_runs;         // cov_run_begin[n_docs] x (begin, end), half-open
    // BED records (bed.hpp), attached by bed(): a reading of the table and of its blocks; whatever replaces either drops them
    bool has_bed = false;
    std::vector<uint64_t> bed_record_begin;   // n_docs + 1: the records of column c are [bed_record_begin[c], bed_record_begin[c + 1])
    std::vector<uint64_t> bed_contig_begin;   // n_docs + 1: the contigs of column c among all contigs
    DevBuf<uint64_t> d_bed_record_begin;      // the same offsets in HBM
    DevBuf<int64_t> d_bed_records;  // bed_record_begin[n_docs] x (contig, rel_start, rel_end, name, strand)
    DevBuf<uint64_t> d_bed_name_begin;        // per contig (and one more): its name in d_bed_names
    DevBuf<char> d_bed_names;
    // contig labels (label.hpp), attached by label(): a reading of the table; whatever replaces the table drops them, new blocks do not
    bool has_label = false, label_names = false;   // label_names: the text carries contig names, not their numbers
    DevBuf<uint32_t> d_label_contig;          // n_rows * n_docs: the contig of the start within its column
    DevBuf<int64_t> d_label_rel;              // n_rows * n_docs: the start inside that contig, -1 for an absent cell
    DevBuf<uint64_t> d_label_contig_begin;    // n_docs + 1: the contigs of column c among all contigs
    DevBuf<uint64_t> d_label_name_begin;      // per contig (and one more): its name in d_label_names (with label_names)
    DevBuf<char> d_label_names;
    // merged thresh / thresh_rev of a string fold (string_fold.hpp): the positions of the rows in their order, a 0 behind every
    // row; whatever replaces the table or its order drops them
    bool has_string_thresh = false;
    size_t string_thresh_len = 0;
    DevBuf<uint16_t> d_string_thresh, d_string_thresh_rev;
    // multi-MUM sequences (sequences.hpp), attached by sequences(): a reading of one column of the table and of a text; whatever
    // replaces the table drops them
    bool has_sequences = false, seq_resident = false, seq_terminator = true;
    int seq_dialect = 0;
    uint64_t seq_text_len = 0, seq_bytes = 0;      // length of the text the sources point into; bytes of all records
    uint64_t seq_text_generation = 0;              // resident: Engine::text_generation() when the records were measured
    DevBuf<uint64_t> d_seq_offset;                 // n_rows + 1: where every record begins
    DevBuf<uint64_t> d_seq_source;                 // n_rows: text position of the record's first forward base (bit 63: reverse)
    DevBuf<uint32_t> d_seq_bases;                  // n_rows: bases written
    DevBuf<uint8_t> d_seq_text;                    // a document handed over, one byte per base in TextRef's byte layout

    MergedRows() = default;
    MergedRows(MergedRows&&) noexcept = default;
    MergedRows& operator=(MergedRows&&) noexcept = default;

    // Which results go when something they read is replaced -- the one place that says so.  Blocks, calls and BED records are
    // row ranges and readings of the blocks; coverage, labels and sequences read the table alone.  (A tool clears its OWN flag on entry.)
    // new blocks (collinear_blocks, set_blocks): calls and BED records go, coverage and labels stay
    void blocks_replaced() { has_calls = false; n_calls = 0; has_bed = false; }
    // a new table or row order (sort_like_direct, collinear_blocks): everything attached goes
    void table_replaced() {
        has_blocks = false; n_blocks = 0; blocks_replaced(); has_coverage = false; has_label = false;
        has_string_thresh = false; string_thresh_len = 0; has_sequences = false;
    }
};

}  // namespace mmt
