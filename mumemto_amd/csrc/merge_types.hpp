// merge_types.hpp -- result of the anchor merge (shared by engine.hpp and merge.hpp).
#pragma once
#include <cstddef>
#include <cstdint>
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

    MergedRows() = default;
    MergedRows(MergedRows&& o) noexcept { *this = std::move(o); }
    MergedRows& operator=(MergedRows&& o) noexcept {
        n_docs = o.n_docs; n_rows = o.n_rows; thresh_len = o.thresh_len; on_host = o.on_host;
        d_length.swap(o.d_length); d_offsets.swap(o.d_offsets); d_strands.swap(o.d_strands); d_thresh.swap(o.d_thresh);
        length = std::move(o.length); offsets = std::move(o.offsets); strands = std::move(o.strands);
        thresh = std::move(o.thresh);
        has_blocks = o.has_blocks; n_blocks = o.n_blocks;
        d_row_block.swap(o.d_row_block); d_blocks.swap(o.d_blocks);
        has_calls = o.has_calls; n_calls = o.n_calls;
        d_calls.swap(o.d_calls);
        has_coverage = o.has_coverage;
        cov_covered = std::move(o.cov_covered); cov_run_begin = std::move(o.cov_run_begin);
        d_run_begin.swap(o.d_run_begin); d_runs.swap(o.d_runs);
        has_bed = o.has_bed;
        bed_record_begin = std::move(o.bed_record_begin); bed_contig_begin = std::move(o.bed_contig_begin);
        d_bed_record_begin.swap(o.d_bed_record_begin); d_bed_records.swap(o.d_bed_records);
        d_bed_name_begin.swap(o.d_bed_name_begin); d_bed_names.swap(o.d_bed_names);
        has_label = o.has_label; label_names = o.label_names;
        d_label_contig.swap(o.d_label_contig); d_label_rel.swap(o.d_label_rel);
        d_label_contig_begin.swap(o.d_label_contig_begin); d_label_name_begin.swap(o.d_label_name_begin);
        d_label_names.swap(o.d_label_names);
        return *this;
    }
};

}  // namespace mmt
