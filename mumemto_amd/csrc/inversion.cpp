// inversion.cpp -- see inversion.hpp.  Stages per batch of columns: (1) the keys of the block heads through the LDS transpose;
// per column that is not ascending: (2) a radix sort of (start, block); (3) the run passes: mark, heads and tails compacted,
// a prefix sum of the '+' flags, one thread per run, the surviving records appended to the calls of the table.
#include "inversion.hpp"

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "collinear_kernels.hpp"
#include "inversion_kernels.hpp"
#include "laps.hpp"
#include "merged_tools.hpp"
#include "prims.hpp"

namespace mmt {
void set_blocks(Engine& e, MergedRows& m, const uint32_t* lr, uint64_t n_blocks) {
    if (m.n_rows > 0xffffffffull)
        throw std::invalid_argument("set blocks: a table of 2^32 rows or more (" + std::to_string(m.n_rows) +
                                    ") is not supported: block lists hold 32-bit row numbers");
    if (n_blocks > m.n_rows) throw std::invalid_argument("set blocks: more blocks (" + std::to_string(n_blocks) + ") than rows (" +
                                                         std::to_string(m.n_rows) + ")");
    if (n_blocks && !lr) throw std::invalid_argument("set blocks: lr must hold 2 x n_blocks entries");
    hipStream_t st = e.stream();
    MMT_HIP(hipSetDevice(e.device()));
    const uint32_t n = (uint32_t)m.n_rows, nd = (uint32_t)m.n_docs, B = (uint32_t)n_blocks;
    DevBuf<uint32_t> blocks, row_block, state;
    blocks.ensure(2 * (size_t)B + 2); row_block.ensure((size_t)n + 1); state.ensure(1);
    MMT_HIP(hipMemsetAsync(state.get(), 0, 4, st));
    if (B) MMT_HIP(hipMemcpyAsync(blocks.get(), lr, (size_t)B * 8, hipMemcpyHostToDevice, st));
    ik::check_table(m.d_offsets.get(), n, nd, state.get(), st);
    ik::check_blocks(blocks.get(), B, n, state.get(), st);
    uint32_t bad = 0;
    MMT_HIP(hipMemcpyAsync(&bad, state.get(), 4, hipMemcpyDeviceToHost, st));
    MMT_HIP(hipStreamSynchronize(st));
    if (bad & ik::BLOCKS_BAD)
        throw std::invalid_argument("set blocks: every block must be (first row, last row) with first <= last < " + std::to_string(n) +
                                    " rows, and the blocks ascending and disjoint");
    if (bad & ik::TABLE_PARTIAL)
        throw std::invalid_argument("set blocks: the table has a partial row (an absent start); blocks are defined over strict "
                                    "multi-MUMs only");
    if (bad & ik::TABLE_UNSORTED)
        throw std::invalid_argument("set blocks: column 0 of the table is not ascending; blocks are row ranges of the sorted table");
    ik::rows_of_blocks(blocks.get(), B, n, row_block.get(), st);
    MMT_HIP(hipStreamSynchronize(st));
    m.d_blocks.swap(blocks); m.d_row_block.swap(row_block);
    m.n_blocks = B;
    m.has_blocks = true;
    m.blocks_replaced();
}

void inversion_calls(Engine& e, MergedRows& m, int64_t max_length, InversionStats* stats) {
    if (!m.has_blocks)
        throw std::runtime_error("inversions: no collinear blocks attached: call mmt_merged_collinear or mmt_merged_set_blocks first");
    hipStream_t st = e.stream();
    MMT_HIP(hipSetDevice(e.device()));
    DevBuf<uint8_t>& temp = e.scratch();
    InversionStats local;
    InversionStats& S = stats ? *stats : local;
    S = InversionStats();
    Laps laps(st, stats ? S.ms : nullptr);
    m.has_calls = false; m.n_calls = 0;
    const uint32_t B = (uint32_t)m.n_blocks, nd = (uint32_t)m.n_docs;
    S.blocks = B;
    grow_keep(m.d_calls, ik::CALL_FIELDS, 0, grow_by_doubling, st);

    // a run is at least two blocks, and column 0 orders the blocks themselves
    if (B >= 2 && nd >= 2) {
        const uint32_t max_runs = B / 2;
        DevBuf<uint64_t> keys, sorted_keys;
        DevBuf<uint32_t> blocks_in, order, plus, plus_sum, heads, tails, sel, count;
        DevBuf<uint8_t> head, tail, keep;
        DevBuf<int64_t> rec;
        ColumnFlags flags;
        sorted_keys.ensure(B); blocks_in.ensure(B); order.ensure(B);
        head.ensure(B); tail.ensure(B); plus.ensure(B); plus_sum.ensure(B);
        heads.ensure((size_t)B + 1); tails.ensure((size_t)B + 1); sel.ensure((size_t)max_runs + 1); keep.ensure((size_t)max_runs + 1);
        rec.ensure((size_t)max_runs * ik::CALL_FIELDS); count.ensure(4);
        // columns of keys, beside the buffers of one sort
        const size_t batch = columns_per_batch(e.device(), nd - 1, (size_t)B * 8, (size_t)B * 24);
        keys.ensure(batch * B);
        flags.ensure(batch);
        ck::iota(blocks_in.get(), B, st);
        for (uint32_t c0 = 1; c0 < nd; c0 += (uint32_t)batch) {
            const uint32_t cols = std::min<uint32_t>((uint32_t)batch, nd - c0);
            laps.begin(0);
            flags.clear(st);
            ck::extract_block_heads(m.d_offsets.get(), m.d_strands.get(), m.d_blocks.get(), B, nd, c0, cols, keys.get(),
                                    flags.state(), flags.key_or_device(), st);
            laps.end();
            flags.read(st);
            if (flags.key_or() >> 63) throw std::runtime_error("inversions: a negative start in the first row of a block");
            const int bits = bit_width_u64(flags.key_or());
            for (uint32_t c = 0; c < cols; c++) {
                if (!flags.descends(c)) { S.cols_ascending++; continue; }      // the identity: every difference is +1
                S.cols_sorted++;
                laps.begin(1);
                prims::sort_pairs_u64_u32(temp, keys.get() + (size_t)c * B, sorted_keys.get(), blocks_in.get(), order.get(), B, 0,
                                          bits, st);
                laps.end();
                laps.begin(2);
                ik::mark(order.get(), sorted_keys.get(), B, head.get(), tail.get(), plus.get(), st);
                prims::select_indices(temp, head.get(), heads.get(), count.get(), B, st);
                prims::select_indices(temp, tail.get(), tails.get(), count.get() + 1, B, st);
                prims::inclusive_sum_u32(temp, plus.get(), plus_sum.get(), B, st);
                uint32_t n_runs[2] = {0, 0};
                MMT_HIP(hipMemcpyAsync(n_runs, count.get(), 8, hipMemcpyDeviceToHost, st));
                MMT_HIP(hipStreamSynchronize(st));
                if (n_runs[0] != n_runs[1] || n_runs[0] > max_runs)
                    throw std::runtime_error("inversions: " + std::to_string(n_runs[0]) + " run heads and " +
                                             std::to_string(n_runs[1]) + " run ends in column " + std::to_string(c0 + c));
                uint32_t kept = 0;
                if (n_runs[0]) {
                    ik::emit(heads.get(), tails.get(), n_runs[0], order.get(), plus_sum.get(), m.d_blocks.get(), m.d_offsets.get(),
                             m.d_length.get(), nd, c0 + c, max_length, rec.get(), keep.get(), st);
                    prims::select_indices(temp, keep.get(), sel.get(), count.get() + 2, n_runs[0], st);
                    MMT_HIP(hipMemcpyAsync(&kept, count.get() + 2, 4, hipMemcpyDeviceToHost, st));
                    MMT_HIP(hipStreamSynchronize(st));
                    if (kept) {
                        grow_keep(m.d_calls, (m.n_calls + kept) * ik::CALL_FIELDS, m.n_calls * ik::CALL_FIELDS, grow_by_doubling, st);
                        ik::compact(rec.get(), sel.get(), kept, m.d_calls.get() + m.n_calls * ik::CALL_FIELDS, st);
                        m.n_calls += kept;
                    }
                }
                laps.end();
                S.runs += n_runs[0];
            }
            MMT_HIP(hipStreamSynchronize(st));            // the keys of this batch are overwritten by the next
            laps.collect();
        }
    } else {
        S.cols_ascending = nd ? nd - 1 : 0;
    }
    MMT_HIP(hipStreamSynchronize(st));
    S.calls = m.n_calls;
    m.has_calls = true;
}

}  // namespace mmt
