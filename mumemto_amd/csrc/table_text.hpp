// table_text.hpp -- device helpers of every kernel that writes table text or looks a position up among contigs: decimals,
// wave sums, the comma-separated fields of a merged-table line, the search over a column's contig ends.  Included by
// rows_kernels.hip, merge_kernels.hip, label_kernels.hip, bed_kernels.hip and density_kernels.hip (wave sums, the row of a
// position) after <hip/hip_runtime.h>.
#pragma once
#include <cstdint>

namespace mmt { namespace tt {

__device__ __forceinline__ uint32_t ndigits(uint64_t v) {
    uint32_t d = 1;
    while (v >= 10) { v /= 10; d++; }
    return d;
}
// the nd digits of v at dst; returns where they end
__device__ __forceinline__ char* put_uint(char* dst, uint64_t v, uint32_t nd) {
    for (uint32_t i = nd; i-- > 0;) { dst[i] = (char)('0' + v % 10); v /= 10; }
    return dst + nd;
}
// width of a signed decimal: optional '-' + digits of |v| (0ull - v: defined for INT64_MIN too)
__device__ __forceinline__ uint32_t int_width(int64_t v) {
    return v < 0 ? 1u + ndigits(0ull - (uint64_t)v) : ndigits((uint64_t)v);
}
__device__ __forceinline__ char* put_int(char* dst, int64_t v) {
    if (v < 0) { *dst++ = '-'; const uint64_t a = 0ull - (uint64_t)v; return put_uint(dst, a, ndigits(a)); }
    return put_uint(dst, (uint64_t)v, ndigits((uint64_t)v));
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { uint32_t w = __shfl_xor(v, o, 64); v = w < v ? w : v; }
    return v;
}
__device__ __forceinline__ uint32_t wave_excl_sum(uint32_t v, uint32_t lane, uint32_t& total) {
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { uint32_t y = __shfl_up(x, o, 64); if (lane >= (uint32_t)o) x += y; }
    total = __shfl(x, 63, 64);
    return x - v;
}

// a field of decimals separated by commas at t + cur, one cell per lane and 64 cells per step; returns where the field ends
template <typename T>
__device__ __forceinline__ uint32_t put_numbers(char* t, uint32_t cur, const T* __restrict__ row, uint32_t n_docs, uint32_t lane) {
    for (uint32_t base = 0; base < n_docs; base += 64) {
        const uint32_t d = base + lane;
        int64_t v = 0; uint32_t cw = 0, wd = 0;
        if (d < n_docs) { v = (int64_t)row[d]; cw = int_width(v); wd = cw + (d + 1 < n_docs ? 1 : 0); }
        uint32_t total;
        const uint32_t at = wave_excl_sum(wd, lane, total);
        if (d < n_docs) {
            char* c = t + cur + at;
            if (v < 0) { c[0] = '-'; put_uint(c + 1, 0ull - (uint64_t)v, cw - 1); } else put_uint(c, (uint64_t)v, cw);
            if (d + 1 < n_docs) c[cw] = ',';
        }
        cur += total;
    }
    return cur;
}
// the strands of a row, + or -, separated by commas at t + cur: 2 * n_docs - 1 bytes; returns where the field ends
__device__ __forceinline__ uint32_t put_strands(char* t, uint32_t cur, const uint8_t* __restrict__ row, uint32_t n_docs, uint32_t lane) {
    for (uint32_t d = lane; d < n_docs; d += 64) {
        t[cur + 2 * d] = row[d] ? '+' : '-';
        if (d + 1 < n_docs) t[cur + 2 * d + 1] = ',';
    }
    return cur + 2 * n_docs - 1;
}

// the first i in [0, cnt) with ends[i] > v, cnt when there is none
__device__ __forceinline__ uint32_t upper_bound(const int64_t* ends, uint32_t cnt, int64_t v) {
    uint32_t lo = 0, hi = cnt;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (ends[mid] > v) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// the last i in [0, n) with at(i) <= v, for an ascending at with at(0) <= v (rows by their first position: row 0 begins at 0)
template <typename At>
__device__ __forceinline__ uint32_t last_at_or_before(uint32_t n, uint64_t v, At at) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (at(mid) <= v) lo = mid; else hi = mid;
    }
    return lo;
}

}}  // namespace mmt::tt
