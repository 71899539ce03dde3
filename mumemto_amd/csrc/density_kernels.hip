// density_kernels.hip -- see density_kernels.hpp.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "density_kernels.hpp"
#include "device_utils.hpp"
#include "launch_grid.hpp"
#include "table_text.hpp"

namespace mmt { namespace dnk {

typedef unsigned long long u64;

constexpr uint32_t BLOCK = 256;
// The workgroup's table in LDS: SLOTS destinations (key = sequence * nbins + bin), claimed by whoever posts to them first and
// kept until the workgroup ends; an event whose slot belongs to another key goes to HBM at once.  24 KB.
constexpr uint32_t SLOTS = 1024, SLOT_BITS = 10;
constexpr u64 NO_KEY = ~0ull;
// workgroups of an add launch: each one flushes up to 2 x SLOTS atomics when it ends
constexpr uint64_t ADD_GRID_CAP = 2048;

// One event of a lane (valid: this lane has one): C[key] += c, E[key] += e.
template <bool PREAGG>
__device__ __forceinline__ void post(bool valid, u64 key, u64 c, u64 e, u64* s_key, u64* s_c, u64* s_e, u64* __restrict__ C,
                                     u64* __restrict__ E) {
    if (!PREAGG) {
        if (valid) { atomicAdd(&C[key], c); atomicAdd(&E[key], e); }
        return;
    }
    if (!valid) return;
    const uint32_t h = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - SLOT_BITS));
    const u64 owner = atomicCAS(&s_key[h], NO_KEY, key);
    if (owner == NO_KEY || owner == key) {
        if (c) atomicAdd(&s_c[h], c);
        if (e) atomicAdd(&s_e[h], e);
    } else {
        if (c) atomicAdd(&C[key], c);
        if (e) atomicAdd(&E[key], e);
    }
}

template <bool PREAGG>
__global__ __launch_bounds__(BLOCK) void k_add(const uint32_t* __restrict__ length, const uint64_t* __restrict__ occ_start,
                                               uint64_t n_rows, const int64_t* __restrict__ starts,
                                               const uint64_t* __restrict__ docs, uint64_t n_occ, int64_t size, uint64_t W,
                                               uint64_t nbins, u64* __restrict__ C, u64* __restrict__ E,
                                               u64* __restrict__ counters) {
    __shared__ u64 s_key[PREAGG ? SLOTS : 1], s_c[PREAGG ? SLOTS : 1], s_e[PREAGG ? SLOTS : 1];
    __shared__ uint64_t s_row[2];
    if (PREAGG) {
        for (uint32_t q = threadIdx.x; q < SLOTS; q += BLOCK) { s_key[q] = NO_KEY; s_c[q] = 0; s_e[q] = 0; }
    }
    uint32_t n_cut = 0, n_empty = 0, n_neg = 0;
    const uint64_t tiles = (n_occ + BLOCK - 1) / BLOCK;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {         // (uniform over the workgroup)
        const uint64_t t0 = t * BLOCK, t1 = t0 + BLOCK < n_occ ? t0 + BLOCK : n_occ;
        __syncthreads();                                      // s_row of the tile before is read; the LDS table is ready
        if (threadIdx.x < 2)
            s_row[threadIdx.x] = tt::last_at_or_before((uint32_t)n_rows, threadIdx.x ? t1 - 1 : t0,
                                                       [&](uint32_t r) { return occ_start[r]; });
        __syncthreads();
        const uint64_t i = t0 + threadIdx.x;
        const bool have = i < t1;
        bool begins = false, ends = false;
        u64 key_a = 0, e_a = 0, key_b = 0, e_b = 0;
        if (have) {
            const uint64_t r0 = s_row[0];
            const uint64_t r = r0 + tt::last_at_or_before((uint32_t)(s_row[1] - r0 + 1), i,
                                                          [&](uint32_t k) { return occ_start[r0 + k]; });
            const int64_t start = starts[i];
            const Slice v = slice_of(start, length[r], size);
            n_cut += v.cut ? 1u : 0u;
            n_neg += start < 0 ? 1u : 0u;
            if (v.a < v.b) {
                const u64 row0 = docs[i] * nbins;
                const u64 ka = (u64)v.a / W;
                const u64 hi_a = (ka + 1) * W < (u64)size ? (ka + 1) * W : (u64)size;
                begins = true; key_a = row0 + ka; e_a = hi_a - (u64)v.a;
                if (v.b < size) {                             // (an interval that ends at `size` has no end event)
                    const u64 kb = (u64)v.b / W;
                    const u64 hi_b = (kb + 1) * W < (u64)size ? (kb + 1) * W : (u64)size;
                    ends = true; key_b = row0 + kb; e_b = 0ull - (hi_b - (u64)v.b);
                }
            } else {
                n_empty++;
            }
        }
        post<PREAGG>(begins, key_a, 1ull, e_a, s_key, s_c, s_e, C, E);
        post<PREAGG>(ends, key_b, ~0ull, e_b, s_key, s_c, s_e, C, E);
    }
    if (PREAGG) {
        __syncthreads();
        for (uint32_t q = threadIdx.x; q < SLOTS; q += BLOCK) {
            const u64 key = s_key[q];
            if (key == NO_KEY) continue;
            if (s_c[q]) atomicAdd(&C[key], s_c[q]);
            if (s_e[q]) atomicAdd(&E[key], s_e[q]);
        }
    }
    const u64 cut = tt::wave_sum(n_cut), empty = tt::wave_sum(n_empty), neg = tt::wave_sum(n_neg);
    if ((threadIdx.x & 63) == 0) {
        if (cut) atomicAdd(&counters[1], cut);
        if (empty) atomicAdd(&counters[2], empty);
        if (neg) atomicAdd(&counters[3], neg);
    }
}
void add(const uint32_t* length, const uint64_t* occ_start, uint64_t n_rows, const int64_t* starts, const uint64_t* docs,
         uint64_t n_occ, int64_t size, uint64_t W, uint64_t nbins, uint64_t* C, uint64_t* E, uint64_t* counters,
         hipStream_t s) {
    if (!n_rows || !n_occ) return;
    hipLaunchKernelGGL(k_add<DENSITY_PREAGG != 0>, dim3(grid_capped(n_occ, BLOCK, ADD_GRID_CAP)), dim3(BLOCK), 0, s, length,
                       occ_start, n_rows, starts, docs, n_occ, size, W, nbins, reinterpret_cast<u64*>(C),
                       reinterpret_cast<u64*>(E), reinterpret_cast<u64*>(counters));
    MMT_HIP(hipGetLastError());
}

__global__ void k_row_base(const uint64_t* __restrict__ sums, uint64_t num, uint64_t nbins, uint64_t* __restrict__ base) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < num; q += stride) base[q] = sums[q * nbins];
}
void row_base(const uint64_t* sums, uint64_t num, uint64_t nbins, uint64_t* base, hipStream_t s) {
    if (!num) return;
    hipLaunchKernelGGL(k_row_base, dim3(grid_capped(num, BLOCK)), dim3(BLOCK), 0, s, sums, num, nbins, base);
    MMT_HIP(hipGetLastError());
}

__global__ void k_finish(const uint64_t* __restrict__ E, const uint64_t* __restrict__ base, uint64_t total, uint64_t nbins,
                         uint64_t size, uint64_t W, uint64_t* out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const uint64_t q = i / nbins, k = i - q * nbins;
        const uint64_t hi = (k + 1) * W < size ? (k + 1) * W : size;
        out[i] = E[i] + (hi - k * W) * (out[i] - base[q]);     // (this work-item alone reads and writes out[i])
    }
}
void finish(const uint64_t* E, const uint64_t* base, uint64_t num, uint64_t nbins, int64_t size, uint64_t W, uint64_t* out,
            hipStream_t s) {
    const uint64_t total = num * nbins;
    if (!total) return;
    hipLaunchKernelGGL(k_finish, dim3(grid_capped(total, BLOCK)), dim3(BLOCK), 0, s, E, base, total, nbins, (uint64_t)size, W, out);
    MMT_HIP(hipGetLastError());
}

}}  // namespace mmt::dnk
