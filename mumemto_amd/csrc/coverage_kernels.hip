// coverage_kernels.hip -- see coverage_kernels.hpp.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "coverage_kernels.hpp"
#include "device_utils.hpp"

namespace mmt { namespace cvk {

// (begin + 1, end + 1) of a cell; (0, 0) for an absent one; (begin + 1, 0) for a dropped one, which so keeps its place in
// the order of the begins
struct Interval { uint64_t b, e; };
__device__ __forceinline__ Interval interval_of(int64_t start, uint32_t len, int64_t seq_len, int64_t min_length) {
    Interval v = {0, 0};
    if (start < 0) return v;                                  // (-1; another negative start is refused by the host through key_or)
    v.b = (uint64_t)start + 1;
    if (start >= seq_len || (int64_t)len < min_length || len == 0) return v;
    const int64_t room = seq_len - start;                      // > 0
    const int64_t end = (int64_t)len < room ? start + (int64_t)len : seq_len;
    v.e = (uint64_t)end + 1;
    return v;
}

// The tile of collinear_kernels.hip's extract_columns, twice: TR rows x TC columns.  Read: the 32 lanes of a half-wave take 32
// consecutive cells of one row (256 contiguous bytes), 8 rows per step.  Write: a wave takes 64 consecutive rows of one column
// (512 contiguous bytes), first of the begins, then of the ends.  Both LDS tiles are [column][row] with one entry of padding
// per column (a stride of 65 entries = 130 dwords across the lanes of the read phase: distinct even banks over a half-wave).
constexpr uint32_t TR = 64, TC = 32;

__global__ __launch_bounds__(256) void k_extract_intervals(const int64_t* __restrict__ off, const uint32_t* __restrict__ length,
                                                           const int64_t* __restrict__ seq_len, uint32_t n, uint32_t n_docs,
                                                           uint32_t c0, uint32_t n_cols, int64_t min_length,
                                                           uint64_t* __restrict__ begins, uint64_t* __restrict__ ends,
                                                           uint32_t* __restrict__ col_state,
                                                           unsigned long long* __restrict__ key_or) {
    __shared__ uint64_t tile_b[TC][TR + 1];
    __shared__ uint64_t tile_e[TC][TR + 1];
    const uint32_t tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t cb = blockIdx.y * TC;
    const uint32_t tiles = (uint32_t)(((uint64_t)n + TR - 1) / TR);
    const bool my_col = cb + tx < n_cols;
    const int64_t my_len = my_col ? seq_len[c0 + cb + tx] : 0;
    uint64_t seen = 0;
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t r0 = (uint64_t)t * TR;
        for (uint32_t i = ty; i < TR; i += 8) {
            const uint64_t r = r0 + i;
            if (r < n && my_col) {
                const int64_t start = off[r * n_docs + c0 + cb + tx];
                const Interval v = interval_of(start, length[r], my_len, min_length);
                seen |= v.b | (start == -1 ? 0ull : (uint64_t)start);
                tile_b[tx][i] = v.b;
                tile_e[tx][i] = v.e;
            }
        }
        __syncthreads();
        for (uint32_t c = wave; c < TC; c += 4) {
            if (cb + c >= n_cols) break;                     // (uniform over the wave)
            const uint64_t r = r0 + lane;
            bool descends = false;
            if (r < n) {
                const uint64_t b = tile_b[c][lane];
                begins[(uint64_t)(cb + c) * n + r] = b;
                ends[(uint64_t)(cb + c) * n + r] = tile_e[c][lane];
                if (r) {
                    const uint64_t before = lane ? tile_b[c][lane - 1]
                                                 : interval_of(off[(r - 1) * n_docs + c0 + cb + c], length[r - 1],
                                                               seq_len[c0 + cb + c], min_length).b;
                    descends = b < before;
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
void extract_intervals(const int64_t* off, const uint32_t* length, const int64_t* seq_len, uint32_t n, uint32_t n_docs,
                       uint32_t c0, uint32_t n_cols, int64_t min_length, uint64_t* begins, uint64_t* ends,
                       uint32_t* col_state, uint64_t* key_or, hipStream_t s) {
    if (!n || !n_cols) return;
    const uint64_t tiles = ((uint64_t)n + TR - 1) / TR;
    const unsigned gx = (unsigned)(tiles < (1u << 18) ? tiles : (1u << 18)), gy = (n_cols + TC - 1) / TC;
    hipLaunchKernelGGL(k_extract_intervals, dim3(gx, gy), dim3(256), 0, s, off, length, seq_len, n, n_docs, c0, n_cols, min_length,
                       begins, ends, col_state, reinterpret_cast<unsigned long long*>(key_or));
    MMT_HIP(hipGetLastError());
}

// ---- the running maximum of 64-bit ends, wave64 -----------------------------------------------------------------------
constexpr uint32_t WAVES = SCAN_BLOCK / 64;

__device__ __forceinline__ uint64_t max_u64(uint64_t a, uint64_t b) { return a > b ? a : b; }

// One round of SCAN_BLOCK consecutive elements, v = this work-item's: the maximum of everything BEFORE the element, where run
// is the maximum of all earlier rounds and tiles; run moves past the round.  Every work-item of the workgroup calls it.
// Inside a wave: an inclusive scan by cross-lane shifts; between the waves: their totals through LDS.
__device__ __forceinline__ uint64_t exclusive_max_round(uint64_t v, uint64_t& run, uint64_t* s_w) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t w = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t y = __shfl_up(w, o, 64);
        if (lane >= (uint32_t)o && y > w) w = y;
    }
    uint64_t before = __shfl_up(w, 1, 64);
    if (lane == 0) before = 0;
    if (lane == 63) s_w[wave] = w;
    __syncthreads();
    uint64_t pre = run, tot = run;
#pragma unroll
    for (uint32_t k = 0; k < WAVES; k++) {
        const uint64_t x = s_w[k];
        if (k < wave) pre = max_u64(pre, x);
        tot = max_u64(tot, x);
    }
    run = tot;
    __syncthreads();                                          // s_w is written again by the next round
    return max_u64(pre, before);
}

__global__ __launch_bounds__(SCAN_BLOCK) void k_tile_max(const uint64_t* __restrict__ ends, uint32_t n,
                                                         uint64_t* __restrict__ tile_max) {
    __shared__ uint64_t s_w[WAVES];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE;
    uint64_t m = 0;
#pragma unroll
    for (uint32_t q = 0; q < SCAN_ITEMS; q++) {                // coalesced: consecutive work-items read consecutive elements
        const uint64_t i = base + (uint64_t)q * SCAN_BLOCK + threadIdx.x;
        if (i < n) m = max_u64(m, ends[i]);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = max_u64(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t r = 0;
        for (uint32_t k = 0; k < WAVES; k++) r = max_u64(r, s_w[k]);
        tile_max[blockIdx.x] = r;
    }
}
void tile_max(const uint64_t* ends, uint32_t n, uint64_t* out, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_tile_max, dim3(scan_tiles(n)), dim3(SCAN_BLOCK), 0, s, ends, n, out);
    MMT_HIP(hipGetLastError());
}

__global__ __launch_bounds__(SCAN_BLOCK) void k_tile_carry(const uint64_t* __restrict__ tile_max, uint32_t tiles,
                                                           uint64_t* __restrict__ carry) {
    __shared__ uint64_t s_w[WAVES];
    uint64_t run = 0;
    for (uint32_t base = 0; base < tiles; base += SCAN_BLOCK) {          // (uniform over the workgroup; tiles < 2^21)
        const uint32_t i = base + threadIdx.x;
        const uint64_t prev = exclusive_max_round(i < tiles ? tile_max[i] : 0ull, run, s_w);
        if (i < tiles) carry[i] = prev;
    }
}
void tile_carry(const uint64_t* tmax, uint32_t tiles, uint64_t* carry, hipStream_t s) {
    if (!tiles) return;
    hipLaunchKernelGGL(k_tile_carry, dim3(1), dim3(SCAN_BLOCK), 0, s, tmax, tiles, carry);
    MMT_HIP(hipGetLastError());
}

__global__ __launch_bounds__(SCAN_BLOCK) void k_apply_prev(const uint64_t* __restrict__ begins, uint64_t* ends,
                                                           const uint64_t* __restrict__ carry, uint32_t n,
                                                           uint32_t* __restrict__ heads, unsigned long long* __restrict__ covered,
                                                           uint32_t* __restrict__ n_heads, uint64_t* __restrict__ col_max) {
    __shared__ uint64_t s_w[WAVES];
    __shared__ uint64_t s_sum[WAVES];
    __shared__ uint32_t s_heads[WAVES];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE;
    uint64_t run = carry[blockIdx.x], sum = 0;
    uint32_t nh = 0;
    for (uint32_t q = 0; q < SCAN_ITEMS; q++) {                // SCAN_ITEMS rounds of SCAN_BLOCK consecutive elements
        const uint64_t i = base + (uint64_t)q * SCAN_BLOCK + threadIdx.x;
        uint64_t b = 0, e = 0;
        if (i < n) { b = begins[i]; e = ends[i]; }
        const uint64_t prev = exclusive_max_round(e, run, s_w);
        if (i < n) {
            const uint32_t head = (e != 0 && b > prev) ? 1u : 0u;   // (a dropped cell, e = 0, never is)
            const uint64_t from = max_u64(b, prev);
            if (e > from) sum += e - from;
            ends[i] = prev;                                    // (this work-item read ends[i] above)
            heads[i] = head;
            nh += head;
        }
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *col_max = run;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { sum += __shfl_xor(sum, o, 64); nh += __shfl_xor(nh, o, 64); }
    if ((threadIdx.x & 63) == 0) { s_sum[threadIdx.x >> 6] = sum; s_heads[threadIdx.x >> 6] = nh; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t total = 0; uint32_t h = 0;
        for (uint32_t k = 0; k < WAVES; k++) { total += s_sum[k]; h += s_heads[k]; }
        if (total) atomicAdd(covered, (unsigned long long)total);
        if (h) atomicAdd(n_heads, h);
    }
}
void apply_prev(const uint64_t* begins, uint64_t* ends, const uint64_t* carry, uint32_t n, uint32_t* heads, uint64_t* covered,
                uint32_t* n_heads, uint64_t* col_max, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_apply_prev, dim3(scan_tiles(n)), dim3(SCAN_BLOCK), 0, s, begins, ends, carry, n, heads,
                       reinterpret_cast<unsigned long long*>(covered), n_heads, col_max);
    MMT_HIP(hipGetLastError());
}

__global__ void k_write_runs(const uint64_t* __restrict__ begins, const uint64_t* __restrict__ prevs,
                             const uint32_t* __restrict__ heads, const uint32_t* __restrict__ numbered, uint32_t n,
                             const uint64_t* __restrict__ col_max, int64_t* __restrict__ runs) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t head = heads[i], r = numbered[i];
        if (head) {
            runs[2 * (uint64_t)r] = (int64_t)(begins[i] - 1);
            if (r) runs[2 * (uint64_t)(r - 1) + 1] = (int64_t)(prevs[i] - 1);      // (an interval lies before it: prev >= 2)
        }
        if (i + 1 == n && r + head) runs[2 * (uint64_t)(r + head - 1) + 1] = (int64_t)(*col_max - 1);
    }
}
void write_runs(const uint64_t* begins, const uint64_t* prevs, const uint32_t* heads, const uint32_t* numbered, uint32_t n,
                const uint64_t* col_max, int64_t* runs, hipStream_t s) {
    if (!n) return;
    const uint64_t g = ((uint64_t)n + 255) / 256;
    hipLaunchKernelGGL(k_write_runs, dim3((unsigned)(g < (1ull << 20) ? g : (1ull << 20))), dim3(256), 0, s, begins, prevs, heads,
                       numbered, n, col_max, runs);
    MMT_HIP(hipGetLastError());
}

}}  // namespace mmt::cvk
