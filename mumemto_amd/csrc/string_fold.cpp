// string_fold.cpp -- see string_fold.hpp.  Stages: (1) split: the pieces of every row of the MUMs of MUMs, the short ones dropped;
// (2) locate and test: the record of every piece in every partition and the three conditions, the failing pieces dropped;
// (3) assemble: the rows over all columns, a radix sort by column 0, one permuting pass; (4) thresholds: the pass over the
// positions.  Between the stages the host reads one count back; nothing of the tables returns to it.
#include "string_fold.hpp"

#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "laps.hpp"
#include "merge_kernels.hpp"
#include "prims.hpp"
#include "string_fold_kernels.hpp"

namespace mmt {
namespace {

const char* const COUNT_MISMATCH = "input # of MUM files does not match merged MUM input file";   // the model's (and the reference's) words

constexpr uint64_t MAX_PIECES = (1ull << 32) - 256;

struct PartUp {
    DevBuf<uint32_t> len;
    DevBuf<int64_t> starts, rec_end;
    DevBuf<uint8_t> strands;
    DevBuf<uint16_t> thresh, thresh_rev;
};

template <typename T>
void upload(DevBuf<T>& dst, const T* src, size_t n, hipStream_t st) {
    dst.ensure(n + 1);
    if (n) MMT_HIP(hipMemcpyAsync(dst.get(), src, n * sizeof(T), hipMemcpyHostToDevice, st));
}

std::string table_name(size_t i, size_t S) { return i < S ? "partition " + std::to_string(i) : std::string("the MUMs of MUMs"); }

}  // namespace

MergedRows string_fold(Engine& e, const mmt_string_part* parts, size_t S, const mmt_string_part* mom, const mmt_string_records* records,
                       StringFoldStats* stats) {
    if (stats) *stats = StringFoldStats();
    if (!parts || !mom || !records) throw std::invalid_argument("string fold: partitions, MUMs of MUMs and records must be non-null");
    if (!S || mom->n_docs != S || records->n_collections != S) throw std::invalid_argument(COUNT_MISMATCH);
    if (S > 0xffffffffull || !sk::thresholds_rows_at_once((uint32_t)S))
        throw std::invalid_argument("string fold: " + std::to_string(S) + " partitions are more than the threshold pass holds");
    if (!records->begin || (records->begin[S] && !records->length)) throw std::invalid_argument("string fold: the record tables must be non-null");
    uint64_t C = 0;
    for (size_t i = 0; i <= S; i++) {
        const mmt_string_part& P = i < S ? parts[i] : *mom;
        if (P.n_rows >= 0xffffffffull)
            throw std::invalid_argument("string fold: " + table_name(i, S) + " has " + std::to_string(P.n_rows) +
                                        " rows: 2^32 - 1 or more are not supported");
        if (P.n_rows && (!P.length || !P.starts || !P.strands)) throw std::invalid_argument("string fold: " + table_name(i, S) + " has a null table");
        if (i == S) break;
        if (!P.n_docs) throw std::invalid_argument("string fold: partition " + std::to_string(i) + " has no columns");
        if (P.thresh_len && (!P.thresh || !P.thresh_rev)) throw std::invalid_argument("string fold: partition " + std::to_string(i) + " has a null threshold table");
        C += P.n_docs;
    }
    if (C > 0xffffffffull) throw std::invalid_argument("string fold: 2^32 columns or more");
    // one past every record of every collection
    std::vector<std::vector<int64_t>> rec_end(S);
    for (size_t i = 0; i < S; i++) {
        const uint64_t b0 = records->begin[i], b1 = records->begin[i + 1];
        if (b1 < b0) throw std::invalid_argument("string fold: the records of collection " + std::to_string(i) + " end before they begin");
        if (b1 - b0 > parts[i].n_rows)
            throw std::invalid_argument("string fold: collection " + std::to_string(i) + " has " + std::to_string(b1 - b0) + " records, partition " +
                                        std::to_string(i) + " only " + std::to_string(parts[i].n_rows) + " rows");
        rec_end[i].resize((size_t)(b1 - b0));
        int64_t sum = 0;
        for (uint64_t k = b0; k < b1; k++) {
            if (records->length[k] < 0)
                throw std::invalid_argument("string fold: record " + std::to_string(k - b0) + " of collection " + std::to_string(i) + " has a negative length");
            rec_end[i][(size_t)(k - b0)] = sum += records->length[k];
        }
    }

    hipStream_t st = e.stream();
    MMT_HIP(hipSetDevice(e.device()));
    DevBuf<uint8_t>& temp = e.scratch();
    StringFoldStats local;
    StringFoldStats& T = stats ? *stats : local;
    Laps laps(st, stats ? T.ms : nullptr);

    // the row tables, and what one pass over each says about them; the thresholds follow when nothing is refused
    std::vector<std::unique_ptr<PartUp>> up(S + 1);
    DevBuf<sk::PartState> d_state;
    d_state.ensure(S + 1);
    MMT_HIP(hipMemsetAsync(d_state.get(), 0, (S + 1) * sizeof(sk::PartState), st));
    for (size_t i = 0; i <= S; i++) {
        const mmt_string_part& P = i < S ? parts[i] : *mom;
        up[i].reset(new PartUp());
        const size_t cells = (size_t)P.n_rows * P.n_docs;
        upload(up[i]->len, P.length, P.n_rows, st);
        upload(up[i]->starts, P.starts, cells, st);
        upload(up[i]->strands, P.strands, cells, st);
        sk::check_table(up[i]->len.get(), up[i]->starts.get(), (uint32_t)P.n_rows, (uint32_t)P.n_docs, d_state.get() + i, st);
    }
    std::vector<sk::PartState> state(S + 1);
    MMT_HIP(hipMemcpyAsync(state.data(), d_state.get(), (S + 1) * sizeof(sk::PartState), hipMemcpyDeviceToHost, st));
    MMT_HIP(hipStreamSynchronize(st));
    for (size_t i = 0; i <= S; i++) {
        if (state[i].flags & sk::PART_ABSENT)
            throw std::invalid_argument("string fold: " + table_name(i, S) + " has an absent start (-1): partial MUMs cannot be merged");
        if (i == S) break;
        if (state[i].flags & sk::PART_UNSORTED)
            throw std::invalid_argument("string fold: the rows of partition " + std::to_string(i) + " are not in the order of their first column "
                                        "(the order its threshold tables are written in)");
        if (state[i].positions != parts[i].thresh_len)
            throw std::invalid_argument("string fold: the threshold tables of partition " + std::to_string(i) + " hold " +
                                        std::to_string(parts[i].thresh_len) + " entries, its rows " + std::to_string(state[i].positions) +
                                        " positions (length + 1 each)");
    }
    const uint32_t nS = (uint32_t)S, m = (uint32_t)mom->n_rows;
    std::vector<sk::PartView> view(S);
    std::vector<uint32_t> col_part;
    for (size_t i = 0; i < S; i++) {
        PartUp& U = *up[i];
        upload(U.thresh, parts[i].thresh, parts[i].thresh_len, st);
        upload(U.thresh_rev, parts[i].thresh_rev, parts[i].thresh_len, st);
        upload(U.rec_end, rec_end[i].data(), rec_end[i].size(), st);
        view[i] = sk::PartView{U.starts.get(), U.strands.get(), U.thresh.get(), U.thresh_rev.get(), U.rec_end.get(), parts[i].thresh_len,
                               (uint32_t)parts[i].n_docs, (uint32_t)col_part.size(), (uint32_t)rec_end[i].size()};
        col_part.insert(col_part.end(), (size_t)parts[i].n_docs, (uint32_t)i);
    }
    DevBuf<sk::PartView> d_parts;
    DevBuf<uint32_t> d_col_part, d_count;
    upload(d_parts, view.data(), S, st);
    upload(d_col_part, col_part.data(), col_part.size(), st);
    d_count.ensure(4);
    const PartUp& M = *up[S];

    // (1) split
    DevBuf<uint32_t> first, pieces, piece_row, kept;
    DevBuf<uint64_t> piece_begin;
    DevBuf<int64_t> seg_len, seg_start;
    DevBuf<uint8_t> keep;
    uint64_t n_pieces = 0;
    uint32_t n_kept = 0;
    laps.begin(0);
    if (m) {
        first.ensure(m); pieces.ensure((size_t)m + 1); piece_begin.ensure((size_t)m + 1);
        MMT_HIP(hipMemsetAsync(pieces.get() + m, 0, 4, st));
        sk::count_pieces(M.len.get(), M.starts.get(), m, nS, view[0].rec_end, view[0].n_rec, first.get(), pieces.get(), st);
        prims::exclusive_sum_u32_to_u64(temp, pieces.get(), piece_begin.get(), (size_t)m + 1, st);
        MMT_HIP(hipMemcpyAsync(&n_pieces, piece_begin.get() + m, 8, hipMemcpyDeviceToHost, st));
        MMT_HIP(hipStreamSynchronize(st));
        if (n_pieces >= MAX_PIECES)             // (a launch over the pieces stays below 2^32 work-items: launch_grid.hpp)
            throw std::invalid_argument("string fold: the MUMs of MUMs are cut into 2^32 - 256 pieces or more (" + std::to_string(n_pieces) + ")");
        const uint32_t np = (uint32_t)n_pieces;
        piece_row.ensure(np); seg_len.ensure(np); seg_start.ensure((size_t)np * S); keep.ensure(np); kept.ensure((size_t)np + 1);
        sk::cut_pieces(M.len.get(), M.starts.get(), M.strands.get(), m, nS, view[0].rec_end, view[0].n_rec, first.get(), piece_begin.get(), np,
                       piece_row.get(), seg_len.get(), seg_start.get(), keep.get(), st);
        prims::select_indices(temp, keep.get(), kept.get(), d_count.get(), np, st);
        n_kept = read_u32(d_count.get(), st);
    }
    laps.end();

    // (2) locate and test
    DevBuf<uint32_t> rec, sel;
    DevBuf<int64_t> left_off, right_off;
    DevBuf<uint8_t> ok, all;
    uint32_t n_sel = 0;
    laps.begin(1);
    if (n_kept) {
        const size_t pairs = (size_t)n_kept * S;
        rec.ensure(pairs); left_off.ensure(pairs); right_off.ensure(pairs); ok.ensure(pairs); all.ensure(n_kept); sel.ensure((size_t)n_kept + 1);
        sk::locate(kept.get(), n_kept, nS, seg_len.get(), seg_start.get(), d_parts.get(), rec.get(), left_off.get(), right_off.get(), ok.get(), st);
        sk::all_ok(ok.get(), n_kept, nS, all.get(), st);
        prims::select_indices(temp, all.get(), sel.get(), d_count.get(), n_kept, st);
        n_sel = read_u32(d_count.get(), st);
    }
    laps.end();
    T.pieces = n_pieces; T.dropped_short = n_pieces - n_kept; T.dropped_thresh = n_kept - n_sel; T.rows = n_sel;

    // (3) assemble, sort by column 0 (stable: equal starts stay in the order of the pieces), permute
    MergedRows out;
    out.n_docs = (size_t)C; out.n_rows = n_sel; out.thresh_len = 0;
    const size_t cells = (size_t)n_sel * (size_t)C;
    out.d_length.ensure((size_t)n_sel + 1); out.d_offsets.ensure(cells + 1); out.d_strands.ensure(cells + 1); out.d_thresh.ensure(1);
    DevBuf<uint32_t> order;
    DevBuf<int64_t> base_fwd, base_rev;
    DevBuf<uint8_t> same;
    laps.begin(2);
    if (n_sel) {
        DevBuf<uint32_t> raw_len, val;
        DevBuf<int64_t> raw_starts;
        DevBuf<uint8_t> raw_strands;
        DevBuf<uint64_t> key, key_sorted, key_or;
        raw_len.ensure(n_sel); raw_starts.ensure(cells); raw_strands.ensure(cells); val.ensure(n_sel); order.ensure(n_sel);
        key.ensure(n_sel); key_sorted.ensure(n_sel); key_or.ensure(1);
        base_fwd.ensure((size_t)n_sel * S); base_rev.ensure((size_t)n_sel * S); same.ensure((size_t)n_sel * S);
        MMT_HIP(hipMemsetAsync(key_or.get(), 0, 8, st));
        sk::assemble(kept.get(), sel.get(), n_sel, nS, (uint32_t)C, d_col_part.get(), d_parts.get(), piece_row.get(), M.strands.get(),
                     seg_len.get(), seg_start.get(), rec.get(), left_off.get(), right_off.get(), raw_len.get(), raw_starts.get(),
                     raw_strands.get(), base_fwd.get(), base_rev.get(), same.get(), key.get(), val.get(), key_or.get(), st);
        uint64_t used = 0;                       // the sort bit range: the bits the OR of column 0 uses
        MMT_HIP(hipMemcpyAsync(&used, key_or.get(), 8, hipMemcpyDeviceToHost, st));
        MMT_HIP(hipStreamSynchronize(st));
        if (used >> 63) { sk::flip_sign(key.get(), n_sel, st); used = ~0ull; }   // a negative start sorts before every other
        prims::sort_pairs_u64_u32(temp, key.get(), key_sorted.get(), val.get(), order.get(), n_sel, 0, bit_width_u64(used), st);
        mk::permute_rows(order.get(), n_sel, (uint32_t)C, raw_len.get(), raw_starts.get(), raw_strands.get(), out.d_length.get(),
                         out.d_offsets.get(), out.d_strands.get(), st);
    }
    laps.end();

    // (4) thresholds
    uint64_t n_out = 0;
    laps.begin(3);
    if (n_sel) {
        DevBuf<uint64_t> row_begin;
        row_begin.ensure((size_t)n_sel + 1);
        MMT_HIP(hipMemsetAsync(out.d_length.get() + n_sel, 0, 4, st));
        prims::exclusive_sum_u32_to_u64(temp, out.d_length.get(), row_begin.get(), (size_t)n_sel + 1, st);
        uint64_t positions = 0;
        MMT_HIP(hipMemcpyAsync(&positions, row_begin.get() + n_sel, 8, hipMemcpyDeviceToHost, st));
        MMT_HIP(hipStreamSynchronize(st));
        n_out = positions + n_sel;
        out.d_string_thresh.ensure((size_t)n_out + 1); out.d_string_thresh_rev.ensure((size_t)n_out + 1);
        sk::thresholds(out.d_length.get(), row_begin.get(), order.get(), n_sel, nS, base_fwd.get(), base_rev.get(), same.get(), d_parts.get(),
                       n_out, out.d_string_thresh.get(), out.d_string_thresh_rev.get(), st);
        laps.end();
        MMT_HIP(hipStreamSynchronize(st));       // (the buffers of this call are read until here)
    } else {
        out.d_string_thresh.ensure(1); out.d_string_thresh_rev.ensure(1);
        laps.end();
        MMT_HIP(hipStreamSynchronize(st));
    }
    laps.collect();
    out.has_string_thresh = true;
    out.string_thresh_len = (size_t)n_out;
    out.on_host = false;
    return out;
}

}  // namespace mmt
