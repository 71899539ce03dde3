// density.cpp -- see density.hpp.  An add is one launch over the flat list of occurrences (events into the tables C and E); a
// finish is one prefix sum of C over the flat table, the sum at the head of every sequence taken aside, and one pass that
// turns the sums into the table of bins in place.
#include "density.hpp"

#include <algorithm>
#include <stdexcept>
#include <string>

#include "density_kernels.hpp"
#include "laps.hpp"
#include "pool.hpp"
#include "prims.hpp"

namespace mmt {

namespace {
constexpr uint64_t MAX_POSITION = 1ull << 40;          // positions are 40 bits wide throughout (wide.hpp)
constexpr size_t BYTES_PER_BIN = 24;                   // C, E and the result
}

Density::Density(Engine& e, const int64_t* seq_lengths, size_t num, uint64_t bin_width) : e_(e), num_(num) {
    if (!seq_lengths) throw std::invalid_argument("mem density: seq_lengths must hold num entries");
    if (num == 0) throw std::invalid_argument("mem density: no sequences (num == 0)");
    if (bin_width == 0) throw std::invalid_argument("mem density: a bin width of 0; bins are 1 position or wider");
    for (size_t c = 0; c < num; c++) {
        if (seq_lengths[c] <= 0 || (uint64_t)seq_lengths[c] > MAX_POSITION)
            throw std::invalid_argument("mem density: sequence " + std::to_string(c) + " has length " +
                                        std::to_string(seq_lengths[c]) + "; lengths are from 1 to 2^40");
        size_ = std::max(size_, seq_lengths[c]);
    }
    W_ = std::min<uint64_t>(bin_width, (uint64_t)size_);
    nbins_ = ((uint64_t)size_ + W_ - 1) / W_;
    MMT_HIP(hipSetDevice(e.device()));
    const size_t avail = pool::available(e.device());
    const unsigned __int128 need = (unsigned __int128)BYTES_PER_BIN * num * nbins_;
    if (need > avail) {
        const uint64_t fit = avail / (BYTES_PER_BIN * num);      // bins per sequence that fit
        std::string msg = "mem density: tables of " + std::to_string(num) + " x " + std::to_string(nbins_) + " bins (" +
                          std::to_string(BYTES_PER_BIN) + " bytes each) exceed the " + std::to_string(avail) +
                          " bytes the device heap can give; ";
        if (fit == 0) msg += "not even one bin per sequence fits";
        else msg += "the smallest --bin that fits is " + std::to_string(((uint64_t)size_ + fit - 1) / fit);
        throw std::invalid_argument(msg);
    }
    const size_t total = num * (size_t)nbins_;
    hipStream_t st = e.stream();
    d_c_.ensure(total); d_e_.ensure(total); d_out_.ensure(total); d_base_.ensure(num); d_counters_.ensure(dnk::N_COUNTERS);
    MMT_HIP(hipMemsetAsync(d_c_.get(), 0, total * 8, st));
    MMT_HIP(hipMemsetAsync(d_e_.get(), 0, total * 8, st));
    MMT_HIP(hipMemsetAsync(d_counters_.get(), 0, dnk::N_COUNTERS * 8, st));
    MMT_HIP(hipStreamSynchronize(st));
}

void Density::add_device(const uint32_t* length, const uint64_t* occ_start, uint64_t n_rows, const int64_t* starts,
                         const uint64_t* docs, uint64_t n_occ) {
    if (!n_rows || !n_occ) return;
    if (n_rows > 0xffffffffull)
        throw std::invalid_argument("mem density: a batch of 2^32 rows or more (" + std::to_string(n_rows) + ") is not supported");
    hipStream_t st = e_.stream();
    Laps laps(st, stats_.ms);
    laps.begin(0);
    dnk::add(length, occ_start, n_rows, starts, docs, n_occ, size_, W_, nbins_, d_c_.get(), d_e_.get(), d_counters_.get(), st);
    laps.end();
    uint64_t h[dnk::N_COUNTERS] = {0, 0, 0, 0};
    MMT_HIP(hipMemcpyAsync(h, d_counters_.get(), sizeof h, hipMemcpyDeviceToHost, st));
    MMT_HIP(hipStreamSynchronize(st));
    laps.collect();
    stats_.occurrences += n_occ;
    stats_.cut = h[1]; stats_.empty = h[2]; stats_.negative = h[3];
    finished_ = false;
}

void Density::add_rows(const uint32_t* length, const uint64_t* occ_start, const int64_t* offsets, const uint64_t* seq_ids,
                       size_t n_rows) {
    if (!length || !occ_start) throw std::invalid_argument("mem density: null row tables (length, occ_start)");
    if (occ_start[0] != 0) throw std::invalid_argument("mem density: occ_start must begin at 0, not " + std::to_string(occ_start[0]));
    for (size_t r = 0; r < n_rows; r++)
        if (occ_start[r + 1] < occ_start[r])
            throw std::invalid_argument("mem density: occ_start is not ascending at row " + std::to_string(r) + " (" +
                                        std::to_string(occ_start[r]) + " then " + std::to_string(occ_start[r + 1]) + ")");
    const uint64_t n_occ = occ_start[n_rows];
    if (n_occ > MAX_POSITION)
        throw std::invalid_argument("mem density: occ_start ends at " + std::to_string(n_occ) + ", beyond 2^40 occurrences");
    if (n_occ && (!offsets || !seq_ids)) throw std::invalid_argument("mem density: null occurrence tables (offsets, seq_ids)");
    for (size_t r = 0; r < n_rows; r++)
        for (uint64_t i = occ_start[r]; i < occ_start[r + 1]; i++)
            if (seq_ids[i] >= num_)
                throw std::invalid_argument("mem density: row " + std::to_string(r) + " has an occurrence in sequence " +
                                            std::to_string(seq_ids[i]) + ", but there are " + std::to_string(num_) +
                                            " sequences (index out of range)");
    if (!n_rows || !n_occ) return;
    MMT_HIP(hipSetDevice(e_.device()));
    hipStream_t st = e_.stream();
    d_length_.ensure(n_rows); d_occ_start_.ensure(n_rows); d_starts_.ensure(n_occ); d_docs_.ensure(n_occ);
    MMT_HIP(hipMemcpyAsync(d_length_.get(), length, n_rows * 4, hipMemcpyHostToDevice, st));
    MMT_HIP(hipMemcpyAsync(d_occ_start_.get(), occ_start, n_rows * 8, hipMemcpyHostToDevice, st));
    MMT_HIP(hipMemcpyAsync(d_starts_.get(), offsets, n_occ * 8, hipMemcpyHostToDevice, st));
    MMT_HIP(hipMemcpyAsync(d_docs_.get(), seq_ids, n_occ * 8, hipMemcpyHostToDevice, st));
    add_device(d_length_.get(), d_occ_start_.get(), n_rows, d_starts_.get(), d_docs_.get(), n_occ);
}

void Density::add_engine(Engine& src) {
    const HostRows& R = src.rows_meta();
    if (R.mum_mode)
        throw std::invalid_argument("mem density: the engine's last run was in MUM mode (or there was none); MEM rows come from a "
                                    "run with max_doc_freq != 1");
    if (src.rows_left_device())
        throw std::invalid_argument("mem density: the engine's last run kept no rows (its text sink wrote and dropped them window "
                                    "by window); run without a sink, or add the rows of its file in batches");
    if (R.n_docs != num_)
        throw std::invalid_argument("mem density: " + std::to_string(num_) + " sequence lengths, but the engine's last run had " +
                                    std::to_string(R.n_docs) + " documents");
    if (src.device() != e_.device())
        throw std::invalid_argument("mem density: the engine's rows are on device " + std::to_string(src.device()) +
                                    ", the tables on device " + std::to_string(e_.device()));
    if (!R.n_rows || !R.n_occ) return;
    MMT_HIP(hipSetDevice(e_.device()));
    if (src.stream() != e_.stream()) MMT_HIP(hipStreamSynchronize(src.stream()));
    const uint32_t* len; const uint64_t *occ_start, *docs; const int64_t* starts;
    src.rows_mem_device(&len, &occ_start, &starts, &docs);
    add_device(len, occ_start, R.n_rows, starts, docs, R.n_occ);
}

void Density::finish() {
    MMT_HIP(hipSetDevice(e_.device()));
    hipStream_t st = e_.stream();
    const size_t total = num_ * (size_t)nbins_;
    stats_.ms[1] = 0;
    Laps laps(st, stats_.ms);
    laps.begin(1);
    prims::exclusive_sum_u64(e_.scratch(), d_c_.get(), d_out_.get(), total, st);
    dnk::row_base(d_out_.get(), num_, nbins_, d_base_.get(), st);
    dnk::finish(d_e_.get(), d_base_.get(), num_, nbins_, size_, W_, d_out_.get(), st);
    laps.end();
    MMT_HIP(hipStreamSynchronize(st));
    laps.collect();
    finished_ = true;
}

void Density::copy_bins(uint64_t* out) const {
    if (!finished_) throw std::invalid_argument("mem density: no table yet: call finish after the last add");
    if (!out) throw std::invalid_argument("mem density: null output table");
    MMT_HIP(hipSetDevice(e_.device()));
    hipStream_t st = e_.stream();
    MMT_HIP(hipMemcpyAsync(out, d_out_.get(), num_ * (size_t)nbins_ * 8, hipMemcpyDeviceToHost, st));
    MMT_HIP(hipStreamSynchronize(st));
}

}  // namespace mmt
