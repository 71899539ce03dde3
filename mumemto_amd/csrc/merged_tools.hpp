// merged_tools.hpp -- host idioms the tools over a merged table share (collinear.cpp, inversion.cpp, coverage.cpp, bed.cpp):
// a record list that grows (the engine's row lists grow by it too), the column batch plan, the per-column flags of a batch.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "device_utils.hpp"
#include "pool.hpp"
#include "switches.hpp"

namespace mmt {

// Room for `need` entries in a list that is appended to; the first `used` entries stay.  A list that has to grow gets
// rule(need, its size now) entries: buffer sizes decide the heap's peak, so the engine's row lists and the tools' record
// lists each keep the rule they were sized with.
inline size_t grow_by_quarter(size_t need, size_t) { return need + need / 4; }               // the engine (engine.cpp)
inline size_t grow_by_doubling(size_t need, size_t size) { return std::max(need, 2 * size); }   // the tools
template <typename T>
inline void grow_keep(DevBuf<T>& list, size_t need, size_t used, size_t (*rule)(size_t, size_t), hipStream_t st) {
    if (need <= list.size()) return;
    DevBuf<T> bigger;
    bigger.ensure(rule(need, list.size()));
    if (used) MMT_HIP(hipMemcpyAsync(bigger.get(), list.get(), used * sizeof(T), hipMemcpyDeviceToDevice, st));
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
