// bed.cpp -- see bed.hpp.  Stages: (1) select: a flag per row, a prefix sum, the two rows and the name of every record -- once
// for a table with blocks, per column for one without (presence differs by column); (2) gather: per batch of columns the
// interval of every record through the LDS transpose; (3) lookup: the contig of every interval; (4) text, on demand per
// column: measure, a 64-bit prefix sum, the lines.
#include "bed.hpp"

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "bed_kernels.hpp"
#include "contig_table.hpp"
#include "laps.hpp"
#include "merged_tools.hpp"
#include "prims.hpp"
#include "text_pieces.hpp"

namespace mmt {
namespace {

// room for `want` records in m.d_bed_records; the first `have` records stay
void reserve_records(MergedRows& m, size_t have, size_t want, hipStream_t st) {
    grow_keep(m.d_bed_records, want * bk::RECORD_FIELDS, have * bk::RECORD_FIELDS, grow_by_doubling, st);
}

// the number of set flags: the last flag and its number
uint32_t count_of(const uint32_t* flag, const uint32_t* number, uint32_t n, hipStream_t st) {
    uint32_t last[2] = {0, 0};
    MMT_HIP(hipMemcpyAsync(&last[0], flag + (n - 1), 4, hipMemcpyDeviceToHost, st));
    MMT_HIP(hipMemcpyAsync(&last[1], number + (n - 1), 4, hipMemcpyDeviceToHost, st));
    MMT_HIP(hipStreamSynchronize(st));
    return last[0] + last[1];
}

void check_column(const MergedRows& m, int64_t col) {
    if (!m.has_bed) throw std::runtime_error("no BED records attached: call mmt_merged_bed first");
    if (col < 0 || col >= (int64_t)m.n_docs)
        throw std::invalid_argument("bed text: column " + std::to_string(col) + " is out of range (0-" +
                                    std::to_string((int64_t)m.n_docs - 1) + ")");
}

// byte offsets of the lines of column col in HBM (n_rec + 1 entries, the last one = all bytes); returns the bytes
uint64_t measure_column(Engine& e, const MergedRows& m, int64_t col, DevBuf<uint64_t>& offset) {
    hipStream_t st = e.stream();
    const size_t r0 = (size_t)m.bed_record_begin[col], n_rec = (size_t)m.bed_record_begin[col + 1] - r0;
    if (!n_rec) return 0;
    DevBuf<uint32_t> bytes;
    bytes.ensure(n_rec + 1); offset.ensure(n_rec + 1);
    bk::measure(m.d_bed_records.get() + r0 * bk::RECORD_FIELDS, (uint32_t)n_rec, m.d_bed_name_begin.get(), m.bed_contig_begin[col],
                bytes.get(), st);
    return line_offsets(e.scratch(), bytes.get(), offset.get(), n_rec, st);
}

// the lines of records [k0, k1) of column col at text[0 ..)
void write_column(Engine& e, const MergedRows& m, int64_t col, const DevBuf<uint64_t>& offset, size_t k0, size_t k1, uint64_t base,
                  char* text) {
    const size_t r0 = (size_t)m.bed_record_begin[col];
    bk::write_lines(m.d_bed_records.get() + (r0 + k0) * bk::RECORD_FIELDS, (uint32_t)(k1 - k0), m.d_bed_name_begin.get(),
                    m.d_bed_names.get(), m.bed_contig_begin[col], offset.get() + k0, base, text, e.stream());
}

}  // namespace

void bed(Engine& e, MergedRows& m, const uint64_t* contig_begin, const int64_t* contig_len, const uint64_t* name_begin,
         const char* names, int64_t seq_idx, int64_t min_single, BedStats* stats) {
    if (m.n_rows > 0xffffffffull)
        throw std::invalid_argument("bed: a table of 2^32 rows or more (" + std::to_string(m.n_rows) + ") is not supported");
    if (seq_idx < -1 || seq_idx >= (int64_t)m.n_docs)
        throw std::invalid_argument("bed: sequence index " + std::to_string(seq_idx) + " is out of range (-1 = all, 0-" +
                                    std::to_string((int64_t)m.n_docs - 1) + ")");
    const uint32_t nd = (uint32_t)m.n_docs, n = (uint32_t)m.n_rows;
    const uint32_t first = seq_idx < 0 ? 0 : (uint32_t)seq_idx, last = seq_idx < 0 ? nd : (uint32_t)seq_idx + 1;
    // the columns asked for are checked
    const ContigTable table = check_contig_table({"bed", first, last, false, true, "\t\n", "an interval"}, nd, contig_begin, contig_len,
                                                 name_begin, names);
    const uint64_t n_contigs = table.n_contigs, name_bytes = table.name_bytes;
    hipStream_t st = e.stream();
    MMT_HIP(hipSetDevice(e.device()));
    DevBuf<uint8_t>& temp = e.scratch();
    BedStats local;
    BedStats& S = stats ? *stats : local;
    S = BedStats();
    Laps laps(st, stats ? S.ms : nullptr);
    m.has_bed = false;
    std::vector<uint64_t> record_begin((size_t)nd + 1, 0);
    size_t n_records = 0;
    reserve_records(m, 0, 1, st);

    // the contig tables: ends and offsets for the lookup (local), names and their offsets for the text (kept with m)
    DevBuf<int64_t> d_ends;
    DevBuf<uint64_t> d_contig_begin, d_clamped;
    d_ends.ensure((size_t)n_contigs + 1); d_contig_begin.ensure((size_t)nd + 1); d_clamped.ensure(1);
    m.d_bed_name_begin.ensure((size_t)n_contigs + 1); m.d_bed_names.ensure((size_t)name_bytes + 1);
    MMT_HIP(hipMemcpyAsync(d_ends.get(), table.ends.data(), ((size_t)n_contigs + 1) * 8, hipMemcpyHostToDevice, st));
    MMT_HIP(hipMemcpyAsync(d_contig_begin.get(), contig_begin, ((size_t)nd + 1) * 8, hipMemcpyHostToDevice, st));
    const uint64_t zero = 0;
    MMT_HIP(hipMemcpyAsync(m.d_bed_name_begin.get(), n_contigs ? name_begin : &zero, ((size_t)n_contigs + 1) * 8,
                           hipMemcpyHostToDevice, st));
    if (name_bytes) MMT_HIP(hipMemcpyAsync(m.d_bed_names.get(), names, (size_t)name_bytes, hipMemcpyHostToDevice, st));
    MMT_HIP(hipMemsetAsync(d_clamped.get(), 0, 8, st));
    MMT_HIP(hipStreamSynchronize(st));

    if (n && first < last) {
        const uint32_t n_cols = last - first;
        DevBuf<uint32_t> flag, present, number, rank, rows;
        DevBuf<int64_t> name, begins, ends_of;
        DevBuf<uint8_t> strands;
        flag.ensure(n); number.ensure(n);
        if (m.has_blocks) {
            // ---- one record list for every column --------------------------------------------------------------------------
            laps.begin(0);
            bk::select_flags(m.d_offsets.get(), m.d_length.get(), m.d_row_block.get(), m.d_blocks.get(), n, nd, 0, min_single,
                             flag.get(), nullptr, st);
            prims::exclusive_sum_u32(temp, flag.get(), number.get(), n, st);
            laps.end();
            const uint32_t n_rec = count_of(flag.get(), number.get(), n, st);
            laps.collect();
            if (n_rec) {
                rows.ensure(2 * (size_t)n_rec); name.ensure(n_rec);
                laps.begin(0);
                bk::list_records(flag.get(), number.get(), nullptr, m.d_row_block.get(), m.d_blocks.get(), n, rows.get(), name.get(), st);
                laps.end();
                flag.release(); number.release();
                reserve_records(m, 0, (size_t)n_cols * n_rec, st);
                const size_t batch = columns_per_batch(e.device(), n_cols, (size_t)n_rec * 17, 0);      // columns of (begin, end, strand)
                begins.ensure(batch * n_rec); ends_of.ensure(batch * n_rec); strands.ensure(batch * n_rec);
                for (uint32_t c0 = first; c0 < last; c0 += (uint32_t)batch) {
                    const uint32_t cols = std::min<uint32_t>((uint32_t)batch, last - c0);
                    laps.begin(1);
                    bk::gather(m.d_offsets.get(), m.d_strands.get(), m.d_length.get(), rows.get(), n_rec, nd, c0, cols, begins.get(),
                               ends_of.get(), strands.get(), st);
                    laps.end();
                    laps.begin(2);
                    bk::lookup(begins.get(), ends_of.get(), strands.get(), name.get(), n_rec, c0, cols, d_contig_begin.get(),
                               d_ends.get(), m.d_bed_records.get() + (size_t)(c0 - first) * n_rec * bk::RECORD_FIELDS,
                               d_clamped.get(), st);
                    laps.end();
                    S.batches++;
                }
                MMT_HIP(hipStreamSynchronize(st));
                laps.collect();
            }
            for (uint32_t c = first; c < last; c++) record_begin[c] = (size_t)(c - first) * n_rec;
            n_records = (size_t)n_cols * n_rec;
        } else {
            // ---- a record list per column: presence decides, and numbers the rows ---------------------------------------------
            present.ensure(n); rank.ensure(n); rows.ensure(2 * (size_t)n); name.ensure(n);
            begins.ensure(n); ends_of.ensure(n); strands.ensure(n);
            for (uint32_t c = first; c < last; c++) {
                laps.begin(0);
                bk::select_flags(m.d_offsets.get(), m.d_length.get(), nullptr, nullptr, n, nd, c, min_single, flag.get(),
                                 present.get(), st);
                prims::exclusive_sum_u32(temp, flag.get(), number.get(), n, st);
                prims::exclusive_sum_u32(temp, present.get(), rank.get(), n, st);
                bk::list_records(flag.get(), number.get(), rank.get(), nullptr, nullptr, n, rows.get(), name.get(), st);
                laps.end();
                const uint32_t n_rec = count_of(flag.get(), number.get(), n, st);
                laps.collect();
                record_begin[c] = n_records;
                if (!n_rec) continue;
                reserve_records(m, n_records, n_records + n_rec, st);
                laps.begin(1);
                bk::gather(m.d_offsets.get(), m.d_strands.get(), m.d_length.get(), rows.get(), n_rec, nd, c, 1, begins.get(),
                           ends_of.get(), strands.get(), st);
                laps.end();
                laps.begin(2);
                bk::lookup(begins.get(), ends_of.get(), strands.get(), name.get(), n_rec, c, 1, d_contig_begin.get(), d_ends.get(),
                           m.d_bed_records.get() + n_records * bk::RECORD_FIELDS, d_clamped.get(), st);
                laps.end();
                S.batches++;
                n_records += n_rec;
                MMT_HIP(hipStreamSynchronize(st));            // the lists of this column are overwritten by the next
                laps.collect();
            }
        }
    }
    for (uint32_t c = last; c <= nd; c++) record_begin[c] = n_records;
    uint64_t clamped = 0;
    m.d_bed_record_begin.ensure((size_t)nd + 1);
    MMT_HIP(hipMemcpyAsync(m.d_bed_record_begin.get(), record_begin.data(), ((size_t)nd + 1) * 8, hipMemcpyHostToDevice, st));
    MMT_HIP(hipMemcpyAsync(&clamped, d_clamped.get(), 8, hipMemcpyDeviceToHost, st));
    MMT_HIP(hipStreamSynchronize(st));
    S.records = n_records;
    S.clamped = clamped;
    m.bed_record_begin = std::move(record_begin);
    m.bed_contig_begin.assign(contig_begin, contig_begin + nd + 1);
    m.has_bed = true;
}

std::string bed_text(Engine& e, const MergedRows& m, int64_t col, BedStats* stats) {
    check_column(m, col);
    hipStream_t st = e.stream();
    MMT_HIP(hipSetDevice(e.device()));
    Laps laps(st, stats ? stats->ms : nullptr);
    DevBuf<uint64_t> offset;
    DevBuf<char> text;
    laps.begin(3);
    const uint64_t bytes = measure_column(e, m, col, offset);
    std::string out((size_t)bytes, '\0');
    if (bytes) {
        text.ensure((size_t)bytes + 1);
        write_column(e, m, col, offset, 0, (size_t)(m.bed_record_begin[col + 1] - m.bed_record_begin[col]), 0, text.get());
    }
    laps.end();
    if (bytes) MMT_HIP(hipMemcpyAsync(&out[0], text.get(), (size_t)bytes, hipMemcpyDeviceToHost, st));
    MMT_HIP(hipStreamSynchronize(st));
    laps.collect();
    if (stats) stats->text_bytes += bytes;
    return out;
}

// pieces of whole lines, each at most this many bytes (a single longer line is a piece of its own); MMT_MERGED_TEXT_PIECE sets it
static constexpr size_t BED_TEXT_PIECE = (size_t)256 << 20;

void bed_write_text(Engine& e, const MergedRows& m, int64_t col, const std::string& path, BedStats* stats) {
    check_column(m, col);
    hipStream_t st = e.stream();
    MMT_HIP(hipSetDevice(e.device()));
    Laps laps(st, stats ? stats->ms : nullptr);
    const size_t n_rec = (size_t)(m.bed_record_begin[col + 1] - m.bed_record_begin[col]);
    DevBuf<uint64_t> offset;
    laps.begin(3);
    const uint64_t bytes = measure_column(e, m, col, offset);
    laps.end();
    write_text_pieces(st, e.device(), offset.get(), n_rec, bytes, text_piece_bytes(BED_TEXT_PIECE), path,
                      [&](size_t k0, size_t k1, uint64_t base, char* dst) { write_column(e, m, col, offset, k0, k1, base, dst); },
                      {&laps, 3, -1});
    if (stats) stats->text_bytes += bytes;
}

}  // namespace mmt
