// coverage.cpp -- see coverage.hpp.  Stages per batch of columns: (1) begins and ends through the LDS transpose, filtered and
// clipped; per column: (2) a radix sort of (begin, end) by begin unless the begins ascend already; (3) the running maximum of
// the ends in three launches, its last one fused with the covered count and the run heads; (4) the heads numbered by a prefix
// sum, every run written by its head and by the head behind it.
#include "coverage.hpp"

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "coverage_kernels.hpp"
#include "laps.hpp"
#include "merged_tools.hpp"
#include "prims.hpp"

namespace mmt {
void coverage(Engine& e, MergedRows& m, const int64_t* seq_lengths, int64_t seq_idx, int64_t min_length, CoverageStats* stats) {
    if (m.n_rows > 0xffffffffull)
        throw std::invalid_argument("coverage: a table of 2^32 rows or more (" + std::to_string(m.n_rows) + ") is not supported");
    if (!seq_lengths) throw std::invalid_argument("coverage: seq_lengths must hold n_docs entries");
    if (seq_idx < -1 || seq_idx >= (int64_t)m.n_docs)
        throw std::invalid_argument("coverage: sequence index " + std::to_string(seq_idx) + " is out of range (-1 = all, 0-" +
                                    std::to_string((int64_t)m.n_docs - 1) + ")");
    const uint32_t nd = (uint32_t)m.n_docs, n = (uint32_t)m.n_rows;
    const uint32_t first = seq_idx < 0 ? 0 : (uint32_t)seq_idx, last = seq_idx < 0 ? nd : (uint32_t)seq_idx + 1;
    for (uint32_t c = first; c < last; c++)
        if (seq_lengths[c] <= 0)
            throw std::invalid_argument("coverage: sequence " + std::to_string(c) + " has length " + std::to_string(seq_lengths[c]) +
                                        "; a coverage is a share of a positive length");
    hipStream_t st = e.stream();
    MMT_HIP(hipSetDevice(e.device()));
    DevBuf<uint8_t>& temp = e.scratch();
    CoverageStats local;
    CoverageStats& S = stats ? *stats : local;
    S = CoverageStats();
    Laps laps(st, stats ? S.ms : nullptr);
    m.has_coverage = false;
    std::vector<uint64_t> covered(nd, 0), run_begin((size_t)nd + 1, 0);
    size_t n_runs = 0;
    grow_keep(m.d_runs, 2, 0, grow_by_doubling, st);

    if (n && first < last) {
        const uint32_t n_cols = last - first, tiles = cvk::scan_tiles(n);
        DevBuf<int64_t> d_len;
        DevBuf<uint64_t> begins, ends, sorted_b, sorted_e, tmax, carry, res;
        DevBuf<uint32_t> heads, numbered;
        ColumnFlags flags;
        d_len.ensure(nd);
        MMT_HIP(hipMemcpyAsync(d_len.get(), seq_lengths, (size_t)nd * 8, hipMemcpyHostToDevice, st));
        MMT_HIP(hipStreamSynchronize(st));
        sorted_b.ensure(n); sorted_e.ensure(n); heads.ensure(n); numbered.ensure(n);
        tmax.ensure(tiles); carry.ensure(tiles);
        // columns of begins and ends, beside the buffers of one column
        const size_t batch = columns_per_batch(e.device(), n_cols, (size_t)n * 16, (size_t)n * 40);
        begins.ensure(batch * n); ends.ensure(batch * n);
        // per column of the batch: covered positions, maximum of the ends (+ 1), run heads
        res.ensure(3 * batch);
        flags.ensure(batch);                         // (the OR is over the begins and the starts)
        for (uint32_t c0 = first; c0 < last; c0 += (uint32_t)batch) {
            const uint32_t cols = std::min<uint32_t>((uint32_t)batch, last - c0);
            laps.begin(0);
            flags.clear(st);
            MMT_HIP(hipMemsetAsync(res.get(), 0, 3 * batch * 8, st));
            cvk::extract_intervals(m.d_offsets.get(), m.d_length.get(), d_len.get(), n, nd, c0, cols, min_length, begins.get(),
                                   ends.get(), flags.state(), flags.key_or_device(), st);
            laps.end();
            flags.read(st);
            laps.collect();
            if (flags.key_or() >> 62) throw std::runtime_error("coverage: a start outside [-1, 2^62) in the table");
            const int bits = bit_width_u64(flags.key_or());
            for (uint32_t c = 0; c < cols; c++) {
                uint64_t* b = begins.get() + (size_t)c * n;
                uint64_t* en = ends.get() + (size_t)c * n;
                uint64_t* r = res.get() + 3 * (size_t)c;
                if (flags.descends(c)) {
                    laps.begin(1);
                    if (prims::sort_pairs_u64_u64_inplace(temp, b, sorted_b.get(), en, sorted_e.get(), n, 0, bits, st)) {
                        b = sorted_b.get(); en = sorted_e.get();
                    }
                    laps.end();
                    S.cols_sorted++;
                } else {
                    S.cols_ascending++;
                }
                laps.begin(2);
                cvk::tile_max(en, n, tmax.get(), st);
                cvk::tile_carry(tmax.get(), tiles, carry.get(), st);
                cvk::apply_prev(b, en, carry.get(), n, heads.get(), r, reinterpret_cast<uint32_t*>(r + 2), r + 1, st);
                laps.end();
                uint64_t h_res[3] = {0, 0, 0};
                MMT_HIP(hipMemcpyAsync(h_res, r, 24, hipMemcpyDeviceToHost, st));
                MMT_HIP(hipStreamSynchronize(st));
                laps.collect();
                covered[c0 + c] = h_res[0];
                run_begin[c0 + c] = n_runs;
                const size_t col_runs = (size_t)(h_res[2] & 0xffffffffull);
                if (col_runs) {
                    grow_keep(m.d_runs, 2 * (n_runs + col_runs), 2 * n_runs, grow_by_doubling, st);
                    laps.begin(3);
                    prims::exclusive_sum_u32(temp, heads.get(), numbered.get(), n, st);
                    cvk::write_runs(b, en, heads.get(), numbered.get(), n, r + 1, m.d_runs.get() + 2 * n_runs, st);
                    laps.end();
                    n_runs += col_runs;
                }
            }
            S.batches++;
            MMT_HIP(hipStreamSynchronize(st));            // the intervals of this batch are overwritten by the next
            laps.collect();
        }
    }
    for (uint32_t c = last; c <= nd; c++) run_begin[c] = n_runs;
    m.d_run_begin.ensure((size_t)nd + 1);
    MMT_HIP(hipMemcpyAsync(m.d_run_begin.get(), run_begin.data(), ((size_t)nd + 1) * 8, hipMemcpyHostToDevice, st));
    MMT_HIP(hipStreamSynchronize(st));
    S.runs = n_runs;
    m.cov_covered = std::move(covered);
    m.cov_run_begin = std::move(run_begin);
    m.has_coverage = true;
}

}  // namespace mmt
