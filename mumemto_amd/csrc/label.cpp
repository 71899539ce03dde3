// label.cpp -- see label.hpp.  Stages: (1) lookup: the contig and the offset of every cell, kept with the table; (2) measure: the
// length of every row's line and a 64-bit prefix sum; (3) write: the lines, whole or in pieces of whole rows; (4) the bytes
// leave the device.  (2)-(4) run again for every text asked for: the block field follows the blocks attached at that time.
#include "label.hpp"

#include <algorithm>
#include <numeric>
#include <stdexcept>
#include <string>
#include <vector>

#include "contig_table.hpp"
#include "label_kernels.hpp"
#include "laps.hpp"
#include "text_pieces.hpp"

namespace mmt {
namespace {

void check_label(const MergedRows& m) {
    if (!m.has_label) throw std::runtime_error("no labels attached: call mmt_merged_label first");
}

const uint32_t* row_block(const MergedRows& m) { return m.has_blocks ? m.d_row_block.get() : nullptr; }

// Where the contig ends of every column are searched: per batch of LABEL_COLS columns the workgroup's LDS pool is dealt out,
// fewest contigs first, to the columns of at most BED_LDS_CONTIGS ends while they fit; the others stay in HBM.
std::vector<uint32_t> stage_plan(const uint64_t* contig_begin, uint32_t nd, uint64_t* in_hbm) {
    std::vector<uint32_t> at(nd, lk::IN_HBM), order;
    for (uint32_t c0 = 0; c0 < nd; c0 += lk::LABEL_COLS) {
        const uint32_t cols = std::min<uint32_t>(lk::LABEL_COLS, nd - c0);
        order.resize(cols);
        std::iota(order.begin(), order.end(), c0);
        auto count = [&](uint32_t c) { return contig_begin[c + 1] - contig_begin[c]; };
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return count(a) < count(b); });
        uint64_t used = 0;
        for (uint32_t c : order) {
            if (count(c) > bk::BED_LDS_CONTIGS || used + count(c) > lk::LABEL_LDS_ENDS) break;
            at[c] = (uint32_t)used;
            used += count(c);
        }
    }
    *in_hbm = (uint64_t)std::count(at.begin(), at.end(), lk::IN_HBM);
    return at;
}

// byte offsets of the lines in HBM (n + 1 entries, the last one = all bytes); returns the bytes
uint64_t measure_rows(Engine& e, const MergedRows& m, DevBuf<uint64_t>& offset) {
    const size_t n = m.n_rows;
    if (!n) return 0;
    hipStream_t st = e.stream();
    DevBuf<uint64_t> bytes;
    bytes.ensure(n + 1); offset.ensure(n + 1);
    lk::measure(m.d_length.get(), m.d_offsets.get(), row_block(m), m.d_label_contig.get(), m.d_label_rel.get(), (uint32_t)n,
                (uint32_t)m.n_docs, m.d_label_contig_begin.get(), m.label_names ? m.d_label_name_begin.get() : nullptr, bytes.get(), st);
    return line_offsets(e.scratch(), bytes.get(), offset.get(), n, st);
}

// the lines of rows [r0, r1) at text[0 ..)
void write_rows(Engine& e, const MergedRows& m, const DevBuf<uint64_t>& offset, size_t r0, size_t r1, uint64_t base, char* text) {
    const size_t nd = m.n_docs;
    lk::write_lines(m.d_length.get() + r0, m.d_offsets.get() + r0 * nd, m.d_strands.get() + r0 * nd,
                    row_block(m) ? row_block(m) + r0 : nullptr, m.d_label_contig.get() + r0 * nd, m.d_label_rel.get() + r0 * nd,
                    (uint32_t)(r1 - r0), (uint32_t)nd, m.d_label_contig_begin.get(),
                    m.label_names ? m.d_label_name_begin.get() : nullptr, m.d_label_names.get(), offset.get() + r0, base, text,
                    e.stream());
}

}  // namespace

void label(Engine& e, MergedRows& m, const uint64_t* contig_begin, const int64_t* contig_len, const uint64_t* name_begin,
           const char* names, bool use_names, LabelStats* stats) {
    m.has_label = false;                         // (a refused call leaves no labels, those of an earlier call included)
    if (stats) *stats = LabelStats();
    if (m.n_rows > 0xffffffffull)
        throw std::invalid_argument("label: a table of 2^32 rows or more (" + std::to_string(m.n_rows) + ") is not supported");
    if (m.n_docs > 0xffffffffull || (m.n_rows && !m.n_docs)) throw std::invalid_argument("label: the table has no columns");
    const uint32_t nd = (uint32_t)m.n_docs, n = (uint32_t)m.n_rows;
    // every column is needed
    const ContigTable table = check_contig_table({"label", 0, nd, true, use_names, "\t\n,", "a start"}, nd, contig_begin, contig_len,
                                                 name_begin, names);
    const uint64_t n_contigs = table.n_contigs, name_bytes = table.name_bytes;
    const std::vector<int64_t>& totals = table.totals;
    uint64_t longest_line = 0;
    for (uint32_t c = 0; c < nd; c++) {
        if (contig_begin[c + 1] - contig_begin[c] > 0xfffffffeull)
            throw std::invalid_argument("label: sequence " + std::to_string(c) + " has 2^32 contigs or more");
        longest_line += table.longest_name[c] + 64;
    }
    if (longest_line >> 31) throw std::invalid_argument("label: a line of 2^31 bytes or more (names of " + std::to_string(longest_line) + " bytes)");
    hipStream_t st = e.stream();
    MMT_HIP(hipSetDevice(e.device()));
    LabelStats local;
    LabelStats& S = stats ? *stats : local;
    S = LabelStats();
    Laps laps(st, stats ? S.ms : nullptr);
    const std::vector<uint32_t> plan = stage_plan(contig_begin, nd, &S.hbm_columns);
    const size_t cells = (size_t)n * nd;

    DevBuf<int64_t> d_ends;
    DevBuf<uint32_t> d_plan;
    DevBuf<uint64_t> d_flags;                    // [0] the first cell beyond its sequence, [1] absent cells
    d_ends.ensure((size_t)n_contigs + 1); d_plan.ensure((size_t)nd + 1); d_flags.ensure(2);
    m.d_label_contig_begin.ensure((size_t)nd + 1);
    m.d_label_name_begin.ensure((size_t)n_contigs + 1); m.d_label_names.ensure((size_t)name_bytes + 1);
    m.d_label_contig.ensure(cells + 1); m.d_label_rel.ensure(cells + 1);
    MMT_HIP(hipMemcpyAsync(d_ends.get(), table.ends.data(), ((size_t)n_contigs + 1) * 8, hipMemcpyHostToDevice, st));
    if (nd) MMT_HIP(hipMemcpyAsync(d_plan.get(), plan.data(), (size_t)nd * 4, hipMemcpyHostToDevice, st));
    MMT_HIP(hipMemcpyAsync(m.d_label_contig_begin.get(), contig_begin, ((size_t)nd + 1) * 8, hipMemcpyHostToDevice, st));
    if (use_names && n_contigs)
        MMT_HIP(hipMemcpyAsync(m.d_label_name_begin.get(), name_begin, ((size_t)n_contigs + 1) * 8, hipMemcpyHostToDevice, st));
    if (name_bytes) MMT_HIP(hipMemcpyAsync(m.d_label_names.get(), names, (size_t)name_bytes, hipMemcpyHostToDevice, st));
    const uint64_t flags0[2] = {lk::NO_CELL, 0};
    MMT_HIP(hipMemcpyAsync(d_flags.get(), flags0, 16, hipMemcpyHostToDevice, st));
    laps.begin(0);
    lk::lookup(m.d_offsets.get(), n, nd, 0, m.d_label_contig_begin.get(), d_ends.get(), d_plan.get(), m.d_label_contig.get(),
               m.d_label_rel.get(), d_flags.get(), d_flags.get() + 1, st);
    laps.end();
    uint64_t flags[2] = {lk::NO_CELL, 0};
    MMT_HIP(hipMemcpyAsync(flags, d_flags.get(), 16, hipMemcpyDeviceToHost, st));
    MMT_HIP(hipStreamSynchronize(st));           // (also: the host tables above are read until here)
    laps.collect();
    if (flags[0] != lk::NO_CELL) {
        int64_t start = 0;
        MMT_HIP(hipMemcpyAsync(&start, m.d_offsets.get() + flags[0], 8, hipMemcpyDeviceToHost, st));
        MMT_HIP(hipStreamSynchronize(st));
        const uint64_t r = flags[0] / nd, c = flags[0] % nd;
        throw std::invalid_argument("label: the start " + std::to_string(start) + " of row " + std::to_string(r) + ", column " +
                                    std::to_string(c) + " lies at or beyond the total length " + std::to_string(totals[c]) +
                                    " of sequence " + std::to_string(c));
    }
    S.cells = cells;
    S.absent = flags[1];
    m.label_names = use_names;
    m.has_label = true;
    DevBuf<uint64_t> offset;
    laps.begin(1);
    S.text_bytes = measure_rows(e, m, offset);
    laps.end();
    MMT_HIP(hipStreamSynchronize(st));
    laps.collect();
}

std::string label_text(Engine& e, const MergedRows& m, LabelStats* stats) {
    check_label(m);
    hipStream_t st = e.stream();
    MMT_HIP(hipSetDevice(e.device()));
    Laps laps(st, stats ? stats->ms : nullptr);
    DevBuf<uint64_t> offset;
    DevBuf<char> text;
    laps.begin(1);
    const uint64_t bytes = measure_rows(e, m, offset);
    laps.end();
    std::string out((size_t)bytes, '\0');
    if (bytes) {
        text.ensure((size_t)bytes + 1);
        laps.begin(2);
        write_rows(e, m, offset, 0, m.n_rows, 0, text.get());
        laps.end();
        laps.begin(3);
        MMT_HIP(hipMemcpyAsync(&out[0], text.get(), (size_t)bytes, hipMemcpyDeviceToHost, st));
        laps.end();
    }
    MMT_HIP(hipStreamSynchronize(st));
    laps.collect();
    if (stats) stats->text_bytes = bytes;
    return out;
}

// pieces of whole rows, each at most this many bytes (a single longer row is a piece of its own); MMT_MERGED_TEXT_PIECE sets it
static constexpr size_t LABEL_TEXT_PIECE = (size_t)1 << 30;

void label_write_text(Engine& e, const MergedRows& m, const std::string& path, LabelStats* stats) {
    check_label(m);
    hipStream_t st = e.stream();
    MMT_HIP(hipSetDevice(e.device()));
    Laps laps(st, stats ? stats->ms : nullptr);
    DevBuf<uint64_t> offset;
    laps.begin(1);
    const uint64_t bytes = measure_rows(e, m, offset);
    laps.end();
    const double wait_ms = write_text_pieces(
        st, e.device(), offset.get(), m.n_rows, bytes, text_piece_bytes(LABEL_TEXT_PIECE), path,
        [&](size_t r0, size_t r1, uint64_t base, char* dst) { write_rows(e, m, offset, r0, r1, base, dst); }, {&laps, 2, 3});
    if (stats) { stats->ms[3] += (float)wait_ms; stats->text_bytes = bytes; }
}

}  // namespace mmt
