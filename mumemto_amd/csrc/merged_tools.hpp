// merged_tools.hpp -- host idioms the tools over a merged table share (collinear.cpp, inversion.cpp, coverage.cpp, bed.cpp):
// the bit range of a sort, a record list that grows, the column batch plan, the per-column flags of a batch.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "device_utils.hpp"
#include "pool.hpp"
#include "switches.hpp"

namespace mmt {

// the bits a radix sort has to look at for keys whose OR is v (at least one)
inline int bit_width_u64(uint64_t v) { int b = 0; while (v) { b++; v >>= 1; } return b ? b : 1; }

// room for `want` entries in a record list that is appended to; the first `have` entries stay
inline void grow_keep(DevBuf<int64_t>& list, size_t have, size_t want, hipStream_t st) {
    if (want <= list.size()) return;
    DevBuf<int64_t> bigger;
    bigger.ensure(std::max(want, 2 * list.size()));
    if (have) MMT_HIP(hipMemcpyAsync(bigger.get(), list.get(), have * 8, hipMemcpyDeviceToDevice, st));
    MMT_HIP(hipStreamSynchronize(st));
    list.swap(bigger);
}

// The batch: as many of the n_cols columns, bytes_per_column each, as half of what the heap has free holds beside the
// buffers of one column's work; MMT_COLLINEAR_BATCH sets it (tests).  At least 1, at most n_cols.
inline size_t columns_per_batch(int device, size_t n_cols, size_t bytes_per_column, size_t bytes_beside) {
    size_t batch = n_cols;
    const size_t avail = pool::available(device) / 2;
    if (n_cols * bytes_per_column + bytes_beside > avail)
        batch = avail > bytes_beside ? (avail - bytes_beside) / bytes_per_column : 1;
    batch = (size_t)sw::num(sw::MMT_COLLINEAR_BATCH, batch);
    return std::min<size_t>(std::max<size_t>(batch, 1), n_cols);
}

// What an extraction kernel reports about a batch of columns: per column 1 = its keys are not ascending; behind them,
// 8-byte aligned, the 64-bit OR of every key.  Both are zero before the kernel runs (clear).
class ColumnFlags {
public:
    void ensure(size_t batch) { or_at_ = (batch + 1) & ~(size_t)1; d_.ensure(or_at_ + 2); h_.resize(or_at_ + 2); }
    void clear(hipStream_t st) { MMT_HIP(hipMemsetAsync(d_.get(), 0, (or_at_ + 2) * 4, st)); }
    uint32_t* state() const { return d_.get(); }
    uint64_t* key_or_device() const { return reinterpret_cast<uint64_t*>(d_.get() + or_at_); }
    // to the host; waits for the stream
    void read(hipStream_t st) {
        MMT_HIP(hipMemcpyAsync(h_.data(), d_.get(), (or_at_ + 2) * 4, hipMemcpyDeviceToHost, st));
        MMT_HIP(hipStreamSynchronize(st));
    }
    bool descends(size_t c) const { return (h_[c] & 1u) != 0; }
    uint64_t key_or() const { return (uint64_t)h_[or_at_] | ((uint64_t)h_[or_at_ + 1] << 32); }

private:
    DevBuf<uint32_t> d_;
    std::vector<uint32_t> h_;
    size_t or_at_ = 0;
};

}  // namespace mmt
