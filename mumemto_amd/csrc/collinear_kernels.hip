// collinear_kernels.hip -- see collinear_kernels.hpp.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "collinear_kernels.hpp"
#include "device_utils.hpp"
#include "launch_grid.hpp"

namespace mmt { namespace ck {

__global__ void k_full_row_flags(const int64_t* __restrict__ off, uint32_t n, uint32_t n_docs, uint8_t* __restrict__ flags) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t r = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; r < n; r += waves) {
        bool absent = false;
        for (uint32_t d = lane; d < n_docs; d += 64) absent |= off[r * n_docs + d] == -1;
        const bool any = __ballot(absent) != 0ull;
        if (lane == 0) flags[r] = any ? 0 : 1;
    }
}
void full_row_flags(const int64_t* off, uint32_t n, uint32_t n_docs, uint8_t* flags, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_full_row_flags, dim3(grid_capped((uint64_t)n * 64, 256)), dim3(256), 0, s, off, n, n_docs, flags);
    MMT_HIP(hipGetLastError());
}

__global__ void k_anchor_keys(const int64_t* __restrict__ off, const uint32_t* __restrict__ rows, uint32_t m, uint32_t n_docs,
                              uint64_t* __restrict__ keys, uint32_t* __restrict__ unsorted) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    bool bad = false;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += stride) {
        const int64_t o = off[(uint64_t)rows[k] * n_docs];
        keys[k] = (uint64_t)o;
        if (k && off[(uint64_t)rows[k - 1] * n_docs] > o) bad = true;
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(unsorted, 1u);
}
void anchor_keys(const int64_t* off, const uint32_t* rows, uint32_t m, uint32_t n_docs, uint64_t* keys, uint32_t* unsorted,
                 hipStream_t s) {
    if (!m) return;
    hipLaunchKernelGGL(k_anchor_keys, dim3(grid_capped(m, 256)), dim3(256), 0, s, off, rows, m, n_docs, keys, unsorted);
    MMT_HIP(hipGetLastError());
}

// A tile is TR items x TC columns; item i is row i of the table, or with BLOCK_HEADS the first row lr[2 i] of block i.  Read:
// the 32 lanes of a half-wave take 32 consecutive cells of one row (256 contiguous bytes), 8 rows per step.  Write: a wave
// takes 64 consecutive items of one column (512 contiguous bytes).  The LDS tile is [column][item] with one key of padding
// per column: the read phase writes with a stride of 65 keys = 130 dwords across lanes (distinct even banks over a
// half-wave), the write phase reads consecutive keys.
constexpr uint32_t TR = 64, TC = 32;

template <bool BLOCK_HEADS>
__device__ __forceinline__ uint64_t row_of(const uint32_t* __restrict__ lr, uint64_t i) {
    return BLOCK_HEADS ? (uint64_t)lr[2 * i] : i;
}

template <bool BLOCK_HEADS>
__global__ __launch_bounds__(256) void k_extract(const int64_t* __restrict__ off, const uint8_t* __restrict__ st,
                                                 const uint32_t* __restrict__ lr, uint32_t n, uint32_t n_docs, uint32_t c0,
                                                 uint32_t n_cols, uint64_t* __restrict__ keys, uint32_t* __restrict__ col_state,
                                                 unsigned long long* __restrict__ key_or) {
    __shared__ uint64_t tile[TC][TR + 1];
    const uint32_t tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t cb = blockIdx.y * TC;
    const uint32_t tiles = (uint32_t)(((uint64_t)n + TR - 1) / TR);
    uint64_t seen = 0;
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t r0 = (uint64_t)t * TR;
        for (uint32_t i = ty; i < TR; i += 8) {
            const uint64_t r = r0 + i;
            if (r < n && cb + tx < n_cols) {
                const uint64_t cell = row_of<BLOCK_HEADS>(lr, r) * n_docs + c0 + cb + tx;
                const uint64_t v = (uint64_t)off[cell];
                seen |= v;
                tile[tx][i] = v | (st[cell] ? STRAND_BIT : 0ull);
            }
        }
        __syncthreads();
        for (uint32_t c = wave; c < TC; c += 4) {
            if (cb + c >= n_cols) break;                     // (uniform over the wave)
            const uint64_t r = r0 + lane;
            bool descends = false;
            if (r < n) {
                const uint64_t key = tile[c][lane];
                keys[(uint64_t)(cb + c) * n + r] = key;
                if (r) {
                    const uint64_t before = lane ? (tile[c][lane - 1] & ~STRAND_BIT)
                                                 : (uint64_t)off[row_of<BLOCK_HEADS>(lr, r - 1) * n_docs + c0 + cb + c];
                    descends = (key & ~STRAND_BIT) < before;
                }
            }
            if (__ballot(descends) != 0ull && lane == 0) atomicOr(&col_state[cb + c], 1u);
        }
        __syncthreads();
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) seen |= __shfl_xor(seen, o, 64);
    if (lane == 0 && seen) atomicOr(key_or, (unsigned long long)seen);
}
template <bool BLOCK_HEADS>
static void extract(const int64_t* off, const uint8_t* st, const uint32_t* lr, uint32_t n, uint32_t n_docs, uint32_t c0,
                    uint32_t n_cols, uint64_t* keys, uint32_t* col_state, uint64_t* key_or, hipStream_t s) {
    if (!n || !n_cols) return;
    const uint64_t tiles = ((uint64_t)n + TR - 1) / TR;
    const unsigned gx = (unsigned)(tiles < (1u << 18) ? tiles : (1u << 18)), gy = (n_cols + TC - 1) / TC;
    hipLaunchKernelGGL(k_extract<BLOCK_HEADS>, dim3(gx, gy), dim3(256), 0, s, off, st, lr, n, n_docs, c0, n_cols, keys, col_state,
                       reinterpret_cast<unsigned long long*>(key_or));
    MMT_HIP(hipGetLastError());
}
void extract_columns(const int64_t* off, const uint8_t* st, uint32_t n, uint32_t n_docs, uint32_t c0, uint32_t n_cols,
                     uint64_t* keys, uint32_t* col_state, uint64_t* key_or, hipStream_t s) {
    extract<false>(off, st, nullptr, n, n_docs, c0, n_cols, keys, col_state, key_or, s);
}
void extract_block_heads(const int64_t* off, const uint8_t* st, const uint32_t* lr, uint32_t n_blocks, uint32_t n_docs, uint32_t c0,
                         uint32_t n_cols, uint64_t* keys, uint32_t* col_state, uint64_t* key_or, hipStream_t s) {
    extract<true>(off, st, lr, n_blocks, n_docs, c0, n_cols, keys, col_state, key_or, s);
}

__global__ void k_iota(uint32_t* __restrict__ v, uint32_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) v[i] = (uint32_t)i;
}
void iota(uint32_t* v, uint32_t n, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_iota, dim3(grid_capped(n, 256)), dim3(256), 0, s, v, n);
    MMT_HIP(hipGetLastError());
}

template <bool IDENTITY>
__global__ void k_adjacency(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ length,
                            uint32_t n, uint32_t* __restrict__ pair_cols, int64_t* __restrict__ pair_gap) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k + 1 < n; k += stride) {
        const uint64_t ka = keys[k], kb = keys[k + 1];
        const uint32_t a = IDENTITY ? (uint32_t)k : perm[k], b = IDENTITY ? (uint32_t)(k + 1) : perm[k + 1];
        const bool plus_a = (ka & STRAND_BIT) != 0, plus_b = (kb & STRAND_BIT) != 0;
        uint32_t pair;
        if (b == a + 1 && plus_a && plus_b) pair = a;
        else if (a == b + 1 && !plus_a && !plus_b) pair = b;
        else continue;
        const int64_t gap = (int64_t)((kb & ~STRAND_BIT) - (ka & ~STRAND_BIT)) - (int64_t)length[a];
        pair_cols[pair] += 1;                                   // the only writer of this pair in this column
        if (gap > pair_gap[pair]) pair_gap[pair] = gap;
    }
}
void adjacency(const uint64_t* keys, const uint32_t* perm, const uint32_t* length, uint32_t n, uint32_t* pair_cols,
               int64_t* pair_gap, hipStream_t s) {
    if (n < 2) return;
    if (perm)
        hipLaunchKernelGGL(k_adjacency<false>, dim3(grid_capped(n - 1, 256)), dim3(256), 0, s, keys, perm, length, n, pair_cols,
                           pair_gap);
    else
        hipLaunchKernelGGL(k_adjacency<true>, dim3(grid_capped(n - 1, 256)), dim3(256), 0, s, keys, perm, length, n, pair_cols,
                           pair_gap);
    MMT_HIP(hipGetLastError());
}

__global__ void k_pair_init(uint32_t* __restrict__ pair_cols, int64_t* __restrict__ pair_gap, uint32_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) { pair_cols[i] = 0; pair_gap[i] = NO_GAP; }
}
void pair_init(uint32_t* pair_cols, int64_t* pair_gap, uint32_t n, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_pair_init, dim3(grid_capped(n, 256)), dim3(256), 0, s, pair_cols, pair_gap, n);
    MMT_HIP(hipGetLastError());
}

struct RowState { bool left, right, single; };
__device__ __forceinline__ RowState row_state(const uint32_t* __restrict__ pair_cols, const int64_t* __restrict__ pair_gap,
                                              const uint32_t* __restrict__ length, uint64_t i, uint32_t n, uint32_t n_docs,
                                              uint32_t max_break, int64_t min_single) {
    auto good = [&](uint64_t p) { return pair_cols[p] == n_docs && (max_break == 0 || pair_gap[p] <= (int64_t)max_break); };
    RowState s;
    s.left = i > 0 && good(i - 1);
    s.right = i + 1 < n && good(i);
    s.single = !s.left && !s.right && min_single >= 0 && (int64_t)length[i] >= min_single;
    return s;
}
__global__ void k_block_starts(const uint32_t* __restrict__ pair_cols, const int64_t* __restrict__ pair_gap,
                               const uint32_t* __restrict__ length, uint32_t n, uint32_t n_docs, uint32_t max_break,
                               int64_t min_single, uint32_t* __restrict__ starts) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const RowState s = row_state(pair_cols, pair_gap, length, i, n, n_docs, max_break, min_single);
        starts[i] = ((s.right && !s.left) || s.single) ? 1u : 0u;
    }
}
void block_starts(const uint32_t* pair_cols, const int64_t* pair_gap, const uint32_t* length, uint32_t n, uint32_t n_docs,
                  uint32_t max_break, int64_t min_single, uint32_t* starts, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_block_starts, dim3(grid_capped(n, 256)), dim3(256), 0, s, pair_cols, pair_gap, length, n, n_docs, max_break,
                       min_single, starts);
    MMT_HIP(hipGetLastError());
}
__global__ void k_block_rows(const uint32_t* __restrict__ pair_cols, const int64_t* __restrict__ pair_gap,
                             const uint32_t* __restrict__ length, const uint32_t* __restrict__ numbered, uint32_t n, uint32_t n_docs,
                             uint32_t max_break, int64_t min_single, uint32_t* __restrict__ row_block, uint32_t* __restrict__ lr) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const RowState s = row_state(pair_cols, pair_gap, length, i, n, n_docs, max_break, min_single);
        const bool member = s.left || s.right || s.single;
        if (!member) { row_block[i] = NO_BLOCK; continue; }
        const uint32_t b = numbered[i] - 1;                    // (a member row lies at or behind the start of its block)
        row_block[i] = b;
        if (!s.left) lr[2 * (uint64_t)b] = (uint32_t)i;
        if (!s.right) lr[2 * (uint64_t)b + 1] = (uint32_t)i;
    }
}
void block_rows(const uint32_t* pair_cols, const int64_t* pair_gap, const uint32_t* length, const uint32_t* numbered, uint32_t n,
                uint32_t n_docs, uint32_t max_break, int64_t min_single, uint32_t* row_block, uint32_t* lr, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_block_rows, dim3(grid_capped(n, 256)), dim3(256), 0, s, pair_cols, pair_gap, length, numbered, n, n_docs,
                       max_break, min_single, row_block, lr);
    MMT_HIP(hipGetLastError());
}

}}  // namespace mmt::ck
