// inversion_kernels.hip -- see inversion_kernels.hpp.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_utils.hpp"
#include "inversion_kernels.hpp"
#include "launch_grid.hpp"

namespace mmt { namespace ik {

__global__ void k_check_table(const int64_t* __restrict__ off, uint32_t n, uint32_t n_docs, uint32_t* __restrict__ state) {
    const uint64_t cells = (uint64_t)n * n_docs, stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t bad = 0;
    for (uint64_t cell = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; cell < cells; cell += stride) {
        const int64_t v = off[cell];
        if (v < 0) bad |= TABLE_PARTIAL;
        const uint64_t r = cell / n_docs;
        if (r && cell == r * n_docs && off[cell - n_docs] > v) bad |= TABLE_UNSORTED;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) bad |= __shfl_xor(bad, o, 64);
    if (bad && (threadIdx.x & 63) == 0) atomicOr(state, bad);
}
void check_table(const int64_t* off, uint32_t n, uint32_t n_docs, uint32_t* state, hipStream_t s) {
    if (!n || !n_docs) return;
    hipLaunchKernelGGL(k_check_table, dim3(grid_capped((uint64_t)n * n_docs, 256)), dim3(256), 0, s, off, n, n_docs, state);
    MMT_HIP(hipGetLastError());
}

__global__ void k_check_blocks(const uint32_t* __restrict__ lr, uint32_t n_blocks, uint32_t n, uint32_t* __restrict__ state) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    bool bad = false;
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < n_blocks; b += stride) {
        const uint32_t l = lr[2 * b], r = lr[2 * b + 1];
        if (l > r || r >= n || (b && l <= lr[2 * b - 1])) bad = true;
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(state, BLOCKS_BAD);
}
void check_blocks(const uint32_t* lr, uint32_t n_blocks, uint32_t n, uint32_t* state, hipStream_t s) {
    if (!n_blocks) return;
    hipLaunchKernelGGL(k_check_blocks, dim3(grid_capped(n_blocks, 256)), dim3(256), 0, s, lr, n_blocks, n, state);
    MMT_HIP(hipGetLastError());
}

__global__ void k_rows_of_blocks(const uint32_t* __restrict__ lr, uint32_t n_blocks, uint32_t n, uint32_t* __restrict__ row_block) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint64_t lo = 0, hi = n_blocks;                          // the number of blocks whose first row is <= i
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (lr[2 * mid] <= i) lo = mid + 1; else hi = mid;
        }
        row_block[i] = (lo && i <= lr[2 * (lo - 1) + 1]) ? (uint32_t)(lo - 1) : 0xffffffffu;
    }
}
void rows_of_blocks(const uint32_t* lr, uint32_t n_blocks, uint32_t n, uint32_t* row_block, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_rows_of_blocks, dim3(grid_capped(n, 256)), dim3(256), 0, s, lr, n_blocks, n, row_block);
    MMT_HIP(hipGetLastError());
}

// A workgroup takes MARK_TILE consecutive positions; their blocks and the three around them (one before, two behind: dec of
// the position before and of the position behind) go through LDS, so that every block number is read from HBM once.
constexpr uint32_t MARK_TILE = MARK_THREADS * MARK_ITEMS;

__global__ __launch_bounds__(MARK_THREADS) void k_mark(const uint32_t* __restrict__ order, const uint64_t* __restrict__ keys,
                                                       uint32_t n_blocks, uint8_t* __restrict__ head, uint8_t* __restrict__ tail,
                                                       uint32_t* __restrict__ plus) {
    __shared__ uint32_t blk[MARK_TILE + 3];                      // blk[t] = order[p0 - 1 + t]
    const uint64_t B = n_blocks;
    const uint64_t tiles = (B + MARK_TILE - 1) / MARK_TILE;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t p0 = t * MARK_TILE;
        for (uint32_t k = threadIdx.x; k < MARK_TILE + 3; k += MARK_THREADS) {
            const uint64_t p = p0 + k;                           // position + 1
            blk[k] = (p >= 1 && p - 1 < B) ? order[p - 1] : 0u;
        }
        __syncthreads();
        // dec of the position at tile slot k (position p0 - 1 + k): both positions exist and the block number falls by one
        auto dec = [&](uint32_t k) {
            const uint64_t p1 = p0 + k;                          // position + 1
            return p1 >= 1 && p1 < B && blk[k] == blk[k + 1] + 1u;   // (a block number is below 2^32 - 1: no wrap)
        };
#pragma unroll
        for (uint32_t it = 0; it < MARK_ITEMS; it++) {
            const uint32_t k = it * MARK_THREADS + threadIdx.x + 1;          // slot of position j
            const uint64_t j = p0 + k - 1;
            if (j < B) {
                const bool d = dec(k), before = dec(k - 1), behind = dec(k + 1);
                head[j] = d && !before;
                tail[j] = d && !behind;
                plus[j] = (keys[j] & STRAND_BIT) ? 1u : 0u;
            }
        }
        __syncthreads();
    }
}
void mark(const uint32_t* order, const uint64_t* keys, uint32_t n_blocks, uint8_t* head, uint8_t* tail, uint32_t* plus,
          hipStream_t s) {
    if (n_blocks < 2) return;
    hipLaunchKernelGGL(k_mark, dim3(grid_capped(n_blocks, MARK_TILE)), dim3(MARK_THREADS), 0, s, order, keys, n_blocks, head, tail,
                       plus);
    MMT_HIP(hipGetLastError());
}

__global__ void k_emit(const uint32_t* __restrict__ heads, const uint32_t* __restrict__ tails, uint32_t n_runs,
                       const uint32_t* __restrict__ order, const uint32_t* __restrict__ plus_sum, const uint32_t* __restrict__ lr,
                       const int64_t* __restrict__ off, const uint32_t* __restrict__ length, uint32_t n_docs, uint32_t col,
                       int64_t max_length, int64_t* __restrict__ rec, uint8_t* __restrict__ keep) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_runs; k += stride) {
        const uint64_t s = heads[k], e = (uint64_t)tails[k] + 1;             // positions s .. e of the column, e < n_blocks
        const uint32_t on_plus = plus_sum[e] - (s ? plus_sum[s - 1] : 0u);
        const uint64_t first = order[s], last = order[e];
        const uint64_t row_a = lr[2 * first + 1], row_b = lr[2 * last];      // last row of the first block, first row of the last
        const int64_t len = (int64_t)length[row_b];
        const int64_t seq_start = off[row_a * n_docs + col], seq_end = off[row_b * n_docs + col] + len;
        int64_t* out = rec + k * CALL_FIELDS;
        out[0] = (int64_t)col;
        out[1] = seq_start;
        out[2] = seq_end;
        out[3] = off[row_a * n_docs];
        out[4] = off[row_b * n_docs] + len;
        const int64_t span = seq_end >= seq_start ? seq_end - seq_start : seq_start - seq_end;
        keep[k] = on_plus == 0 && (max_length < 0 || span <= max_length);
    }
}
void emit(const uint32_t* heads, const uint32_t* tails, uint32_t n_runs, const uint32_t* order, const uint32_t* plus_sum,
          const uint32_t* lr, const int64_t* off, const uint32_t* length, uint32_t n_docs, uint32_t col, int64_t max_length,
          int64_t* rec, uint8_t* keep, hipStream_t s) {
    if (!n_runs) return;
    hipLaunchKernelGGL(k_emit, dim3(grid_capped(n_runs, 256)), dim3(256), 0, s, heads, tails, n_runs, order, plus_sum, lr, off,
                       length, n_docs, col, max_length, rec, keep);
    MMT_HIP(hipGetLastError());
}

__global__ void k_compact(const int64_t* __restrict__ rec, const uint32_t* __restrict__ sel, uint32_t n_sel, int64_t* __restrict__ out) {
    const uint64_t items = (uint64_t)n_sel * CALL_FIELDS, stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += stride) {
        const uint64_t k = i / CALL_FIELDS, f = i - k * CALL_FIELDS;
        out[i] = rec[(uint64_t)sel[k] * CALL_FIELDS + f];
    }
}
void compact(const int64_t* rec, const uint32_t* sel, uint32_t n_sel, int64_t* out, hipStream_t s) {
    if (!n_sel) return;
    hipLaunchKernelGGL(k_compact, dim3(grid_capped((uint64_t)n_sel * CALL_FIELDS, 256)), dim3(256), 0, s, rec, sel, n_sel, out);
    MMT_HIP(hipGetLastError());
}

}}  // namespace mmt::ik
