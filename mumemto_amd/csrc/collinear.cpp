// collinear.cpp -- see collinear.hpp.  Stages: (1) partial rows out, rows into ascending order of column 0; (2) per batch of
// columns: keys through the LDS transpose, a radix sort of (start, row) for every column that is not ascending already, one
// adjacency pass per column; (3) block heads from the per-pair results, numbered by a prefix sum.
#include "collinear.hpp"

#include <algorithm>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "collinear_kernels.hpp"
#include "laps.hpp"
#include "merge_kernels.hpp"
#include "merged_tools.hpp"
#include "prims.hpp"

namespace mmt {
void collinear_blocks(Engine& e, MergedRows& m, uint32_t max_break, int64_t min_single, CollinearStats* stats) {
    if (m.n_rows > 0xffffffffull)
        throw std::runtime_error("collinear blocks: a table of 2^32 rows or more (" + std::to_string(m.n_rows) +
                                 ") is not supported: block lists hold 32-bit row numbers");
    if (!m.n_docs) throw std::runtime_error("collinear blocks: a table without columns");
    hipStream_t st = e.stream();
    MMT_HIP(hipSetDevice(e.device()));
    DevBuf<uint8_t>& temp = e.scratch();
    const uint32_t nd = (uint32_t)m.n_docs;
    CollinearStats local;
    CollinearStats& S = stats ? *stats : local;
    S = CollinearStats();
    Laps laps(st, stats ? S.ms : nullptr);
    m.table_replaced();                          // (this call filters and sorts the table)
    S.rows_in = m.n_rows;

    // ---- (1) MUMdata.filter_pmums + MUMdata.sort (utils.py:486-495, :323-361) -------------------------------------------
    uint32_t n = (uint32_t)m.n_rows;
    if (n) {
        DevBuf<uint8_t> flags;
        DevBuf<uint32_t> idx, idx2, count;
        DevBuf<uint64_t> key_a, key_b;
        flags.ensure((size_t)n + 1); idx.ensure((size_t)n + 1); count.ensure(4);
        laps.begin(0);
        MMT_HIP(hipMemsetAsync(count.get(), 0, 16, st));
        ck::full_row_flags(m.d_offsets.get(), n, nd, flags.get(), st);
        prims::select_indices(temp, flags.get(), idx.get(), count.get(), n, st);
        uint32_t kept = 0, unsorted = 0;
        MMT_HIP(hipMemcpyAsync(&kept, count.get(), 4, hipMemcpyDeviceToHost, st));
        MMT_HIP(hipStreamSynchronize(st));
        flags.release();
        if (kept) {
            key_a.ensure((size_t)kept + 1);
            ck::anchor_keys(m.d_offsets.get(), idx.get(), kept, nd, key_a.get(), count.get() + 1, st);
            MMT_HIP(hipMemcpyAsync(&unsorted, count.get() + 1, 4, hipMemcpyDeviceToHost, st));
            MMT_HIP(hipStreamSynchronize(st));
            if (unsorted) {             // stable: equal starts keep the order of their rows
                key_b.ensure((size_t)kept + 1); idx2.ensure((size_t)kept + 1);
                prims::sort_pairs_u64_u32(temp, key_a.get(), key_b.get(), idx.get(), idx2.get(), kept, 0, 64, st);
                idx.swap(idx2);
                S.table_sorted = 1;
            }
        }
        if (kept < n || unsorted) {
            DevBuf<uint32_t> len2; DevBuf<int64_t> off2; DevBuf<uint8_t> st2;
            len2.ensure((size_t)kept + 1); off2.ensure((size_t)kept * nd + 1); st2.ensure((size_t)kept * nd + 1);
            mk::permute_rows(idx.get(), kept, nd, m.d_length.get(), m.d_offsets.get(), m.d_strands.get(), len2.get(), off2.get(),
                             st2.get(), st);
            MMT_HIP(hipStreamSynchronize(st));
            m.d_length.swap(len2); m.d_offsets.swap(off2); m.d_strands.swap(st2);
            m.n_rows = kept;
            m.on_host = false;
            m.length.clear(); m.offsets.clear(); m.strands.clear();
        }
        laps.end();
        MMT_HIP(hipStreamSynchronize(st));
        laps.collect();
        n = kept;
    }
    S.rows_kept = n;

    // ---- (2) which pairs (i, i + 1) are collinear --------------------------------------------------------------------
    DevBuf<uint32_t> pair_cols; DevBuf<int64_t> pair_gap;
    pair_cols.ensure((size_t)n + 1); pair_gap.ensure((size_t)n + 1);
    ck::pair_init(pair_cols.get(), pair_gap.get(), n, st);
    if (n >= 2) {
        DevBuf<uint64_t> keys, sorted_keys;
        DevBuf<uint32_t> rows_in, rows_out;
        ColumnFlags flags;
        sorted_keys.ensure(n); rows_in.ensure(n); rows_out.ensure(n);
        // columns of keys, beside the buffers of one sort
        const size_t batch = columns_per_batch(e.device(), nd, (size_t)n * 8, (size_t)n * 24);
        keys.ensure(batch * n);
        flags.ensure(batch);
        ck::iota(rows_in.get(), n, st);
        for (uint32_t c0 = 0; c0 < nd; c0 += (uint32_t)batch) {
            const uint32_t cols = std::min<uint32_t>((uint32_t)batch, nd - c0);
            laps.begin(1);
            flags.clear(st);
            ck::extract_columns(m.d_offsets.get(), m.d_strands.get(), n, nd, c0, cols, keys.get(), flags.state(),
                                flags.key_or_device(), st);
            laps.end();
            flags.read(st);
            if (flags.key_or() >> 63) throw std::runtime_error("collinear blocks: a negative start other than -1 in the table");
            const int bits = bit_width_u64(flags.key_or());
            for (uint32_t c = 0; c < cols; c++) {
                const uint64_t* col = keys.get() + (size_t)c * n;
                if (flags.descends(c)) {
                    laps.begin(2);
                    prims::sort_pairs_u64_u32(temp, col, sorted_keys.get(), rows_in.get(), rows_out.get(), n, 0, bits, st);
                    laps.end();
                    laps.begin(3);
                    ck::adjacency(sorted_keys.get(), rows_out.get(), m.d_length.get(), n, pair_cols.get(), pair_gap.get(), st);
                    laps.end();
                    S.cols_sorted++;
                } else {
                    laps.begin(3);
                    ck::adjacency(col, nullptr, m.d_length.get(), n, pair_cols.get(), pair_gap.get(), st);
                    laps.end();
                    S.cols_ascending++;
                }
            }
            S.batches++;
            MMT_HIP(hipStreamSynchronize(st));            // the keys of this batch are overwritten by the next
            laps.collect();
        }
    }

    // ---- (3) blocks ----------------------------------------------------------------------------------------------------
    m.d_row_block.ensure((size_t)n + 1);
    uint32_t n_blocks = 0;
    if (n) {
        DevBuf<uint32_t> starts, numbered;
        starts.ensure(n); numbered.ensure(n);
        laps.begin(4);
        ck::block_starts(pair_cols.get(), pair_gap.get(), m.d_length.get(), n, nd, max_break, min_single, starts.get(), st);
        prims::inclusive_sum_u32(temp, starts.get(), numbered.get(), n, st);
        MMT_HIP(hipMemcpyAsync(&n_blocks, numbered.get() + (n - 1), 4, hipMemcpyDeviceToHost, st));
        MMT_HIP(hipStreamSynchronize(st));
        m.d_blocks.ensure(2 * (size_t)n_blocks + 2);
        ck::block_rows(pair_cols.get(), pair_gap.get(), m.d_length.get(), numbered.get(), n, nd, max_break, min_single,
                       m.d_row_block.get(), m.d_blocks.get(), st);
        laps.end();
        MMT_HIP(hipStreamSynchronize(st));
        laps.collect();
    } else {
        m.d_blocks.ensure(2);
    }
    m.n_blocks = n_blocks;
    m.has_blocks = true;
}

}  // namespace mmt
