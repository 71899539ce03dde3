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
#include "laps.hpp"
#include "piece_writer.hpp"
#include "pool.hpp"
#include "prims.hpp"
#include "switches.hpp"

namespace mmt {
namespace {

constexpr size_t REC_BYTES = bk::RECORD_FIELDS * 8;

// room for `want` records in m.d_bed_records; the first `have` records stay
void reserve_records(MergedRows& m, size_t have, size_t want, hipStream_t st) {
    if (want * bk::RECORD_FIELDS <= m.d_bed_records.size()) return;
    DevBuf<int64_t> bigger;
    bigger.ensure(std::max(want * bk::RECORD_FIELDS, 2 * m.d_bed_records.size()));
    if (have) MMT_HIP(hipMemcpyAsync(bigger.get(), m.d_bed_records.get(), have * REC_BYTES, hipMemcpyDeviceToDevice, st));
    MMT_HIP(hipStreamSynchronize(st));
    m.d_bed_records.swap(bigger);
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
    MMT_HIP(hipMemsetAsync(bytes.get() + n_rec, 0, 4, st));
    prims::exclusive_sum_u32_to_u64(e.scratch(), bytes.get(), offset.get(), n_rec + 1, st);
    uint64_t total = 0;
    MMT_HIP(hipMemcpyAsync(&total, offset.get() + n_rec, 8, hipMemcpyDeviceToHost, st));
    MMT_HIP(hipStreamSynchronize(st));
    return total;
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
    if (!contig_begin) throw std::invalid_argument("bed: contig_begin must hold n_docs + 1 entries");
    const uint32_t nd = (uint32_t)m.n_docs, n = (uint32_t)m.n_rows;
    for (uint32_t c = 0; c < nd; c++)
        if (contig_begin[c] > contig_begin[c + 1]) throw std::invalid_argument("bed: contig_begin does not ascend");
    const uint64_t n_contigs = contig_begin[nd];
    if (n_contigs && (!contig_len || !name_begin))
        throw std::invalid_argument("bed: contig_len and name_begin must hold an entry per contig (name_begin one more)");
    for (uint64_t g = 0; g < n_contigs; g++)
        if (name_begin[g] > name_begin[g + 1]) throw std::invalid_argument("bed: name_begin does not ascend");
    const uint64_t name_bytes = n_contigs ? name_begin[n_contigs] : 0;
    if (name_bytes && !names) throw std::invalid_argument("bed: names must hold the bytes name_begin refers to");
    const uint32_t first = seq_idx < 0 ? 0 : (uint32_t)seq_idx, last = seq_idx < 0 ? nd : (uint32_t)seq_idx + 1;
    // cumulative lengths per column; the columns asked for are checked
    std::vector<int64_t> ends((size_t)n_contigs + 1, 0);
    for (uint32_t c = 0; c < nd; c++) {
        const bool needed = c >= first && c < last;
        if (needed && contig_begin[c] == contig_begin[c + 1])
            throw std::invalid_argument("bed: sequence " + std::to_string(c) + " has no contigs");
        uint64_t run = 0;
        for (uint64_t g = contig_begin[c]; g < contig_begin[c + 1]; g++) {
            if (needed && contig_len[g] < 0)
                throw std::invalid_argument("bed: contig " + std::to_string(g - contig_begin[c]) + " of sequence " + std::to_string(c) +
                                            " has the negative length " + std::to_string(contig_len[g]));
            run += (uint64_t)contig_len[g];
            if (needed && run >> 62) throw std::invalid_argument("bed: sequence " + std::to_string(c) + " is 2^62 bases or longer");
            ends[g] = (int64_t)run;
            if (!needed) continue;
            for (uint64_t i = name_begin[g]; i < name_begin[g + 1]; i++)
                if (names[i] == '\t' || names[i] == '\n')
                    throw std::invalid_argument("bed: the name of contig " + std::to_string(g - contig_begin[c]) + " of sequence " +
                                                std::to_string(c) + " contains a tab or a newline");
        }
        if (needed && run == 0)
            throw std::invalid_argument("bed: sequence " + std::to_string(c) + " has total length 0: no contig can hold an interval");
    }
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
    MMT_HIP(hipMemcpyAsync(d_ends.get(), ends.data(), ((size_t)n_contigs + 1) * 8, hipMemcpyHostToDevice, st));
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
                // the batch: as many columns of (begin, end, strand) as half of what the heap has free holds
                size_t batch = n_cols;
                const size_t avail = pool::available(e.device()) / 2, one_col = (size_t)n_rec * 17;
                if (batch * one_col > avail) batch = avail / one_col;
                batch = (size_t)sw::num(sw::MMT_COLLINEAR_BATCH, batch);
                batch = std::min<size_t>(std::max<size_t>(batch, 1), n_cols);
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

// pieces of whole lines, each at most this many bytes (a single longer line is a piece of its own)
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
    std::vector<size_t> cut(1, 0);
    std::vector<uint64_t> h_off;
    uint64_t longest = 0;
    if (bytes <= BED_TEXT_PIECE) {
        if (bytes) cut.push_back(n_rec);
        h_off = {0, bytes};
        longest = bytes;
    } else {
        h_off.resize(n_rec + 1);
        MMT_HIP(hipMemcpyAsync(h_off.data(), offset.get(), (n_rec + 1) * 8, hipMemcpyDeviceToHost, st));
        MMT_HIP(hipStreamSynchronize(st));
        for (size_t r = 0; r < n_rec;) {
            const uint64_t lim = h_off[r] + BED_TEXT_PIECE;
            size_t q = (size_t)(std::upper_bound(h_off.begin() + r + 1, h_off.end(), lim) - h_off.begin()) - 1;
            if (q <= r) q = r + 1;
            longest = std::max<uint64_t>(longest, h_off[q] - h_off[r]);
            cut.push_back(q);
            r = q;
        }
    }
    const bool one = bytes <= BED_TEXT_PIECE;
    DevBuf<char> d_piece[2];
    for (auto& d : d_piece) d.ensure((size_t)longest + 1);
    PieceWriter writer((size_t)longest + 1, 2);
    writer.open(path, e.device(), false);        // (left open by an exception: its destructor removes PATH.tmp)
    for (size_t i = 0; i + 1 < cut.size(); i++) {
        DevBuf<char>& d = d_piece[i & 1];
        const size_t k0 = cut[i], k1 = cut[i + 1];
        const uint64_t from = one ? 0 : h_off[k0], to = one ? bytes : h_off[k1];
        PieceWriter::Piece pc = writer.room((size_t)(to - from));
        laps.begin(3);
        write_column(e, m, col, offset, k0, k1, from, d.get());
        laps.end();
        MMT_HIP(hipMemcpyAsync(pc.p, d.get(), pc.n, hipMemcpyDeviceToHost, st));
        MMT_HIP(hipStreamSynchronize(st));
        writer.push(pc);
    }
    MMT_HIP(hipStreamSynchronize(st));
    laps.collect();
    writer.close();
    if (stats) stats->text_bytes += bytes;
}

}  // namespace mmt
