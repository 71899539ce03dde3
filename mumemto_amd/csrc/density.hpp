// density.hpp -- MEM density of the sequences on the device (the reference's mumemto/mem_density.py:20-39: for every
// occurrence of every row, `coverage[idx, start:start+l] += 1` in a num x max(seq_lengths) array of float64), in bins of W
// positions: W = 1 is the reference's array, a larger W fits whole genomes.  Kernels and the closed form:
// density_kernels.hpp.
#pragma once
#include <cstddef>
#include <cstdint>

#include "engine.hpp"

namespace mmt {

struct DensityStats {
    float ms[2] = {0, 0};              // HIP-event milliseconds: every add pass so far, the last finish pass
    // occurrences added; of them: with start + length beyond `size` (cut there), that covered nothing, with a negative start
    uint64_t occurrences = 0, cut = 0, empty = 0, negative = 0;
};

class Density {
public:
    // seq_lengths: num host entries; size = their maximum.  bin_width beyond size means one bin per sequence.  Throws
    // std::invalid_argument for a null seq_lengths, num == 0, a length <= 0 or beyond 2^40, bin_width == 0 and tables that the
    // device heap cannot hold: the two event tables and the result, 24 x num x nbins bytes, beside the scan's scratch.
    Density(Engine& e, const int64_t* seq_lengths, size_t num, uint64_t bin_width);

    // A host batch of whole rows: length[n_rows], occ_start[n_rows + 1] (from 0, ascending, at most 2^40), offsets and
    // seq_ids[occ_start[n_rows]].  Everything is checked before anything is launched (std::invalid_argument).
    void add_rows(const uint32_t* length, const uint64_t* occ_start, const int64_t* offsets, const uint64_t* seq_ids,
                  size_t n_rows);
    // the MEM rows of src's last run, read where they lie in HBM; src must be on this density's device
    void add_engine(Engine& src);
    // the table of sums from the events posted so far; adding goes on from there afterwards
    void finish();

    size_t num() const { return num_; }
    uint64_t nbins() const { return nbins_; }
    int64_t size() const { return size_; }
    uint64_t bin_width() const { return W_; }
    bool finished() const { return finished_; }
    const uint64_t* bins_device() const { return d_out_.get(); }      // num x nbins, after finish()
    void copy_bins(uint64_t* out) const;
    const DensityStats& stats() const { return stats_; }

private:
    void add_device(const uint32_t* length, const uint64_t* occ_start, uint64_t n_rows, const int64_t* starts,
                    const uint64_t* docs, uint64_t n_occ);
    Engine& e_;
    size_t num_ = 0;
    int64_t size_ = 0;
    uint64_t W_ = 1, nbins_ = 0;
    bool finished_ = false;
    DevBuf<uint64_t> d_c_, d_e_, d_out_, d_base_, d_counters_, d_occ_start_, d_docs_;
    DevBuf<int64_t> d_starts_;
    DevBuf<uint32_t> d_length_;
    DensityStats stats_;
};

}  // namespace mmt
