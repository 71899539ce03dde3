// label_kernels.hip -- see label_kernels.hpp.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_utils.hpp"
#include "label_kernels.hpp"
#include "launch_grid.hpp"
#include "table_text.hpp"

namespace mmt { namespace lk {

using namespace tt;      // the decimals, wave sums, field writers and the contig search

// ---- contig lookup --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LABEL_BLOCK) void k_lookup(const int64_t* __restrict__ off, uint32_t n, uint32_t n_docs, uint64_t row0,
                                                        const uint64_t* __restrict__ contig_begin,
                                                        const int64_t* __restrict__ ends, const uint32_t* __restrict__ stage_at,
                                                        uint32_t* __restrict__ contig, int64_t* __restrict__ rel,
                                                        unsigned long long* __restrict__ beyond,
                                                        unsigned long long* __restrict__ absent) {
    __shared__ int64_t s_ends[LABEL_LDS_ENDS];
    __shared__ uint64_t s_first[LABEL_COLS];
    __shared__ uint32_t s_cnt[LABEL_COLS], s_at[LABEL_COLS];
    const uint32_t c0 = blockIdx.y * LABEL_COLS;                               // (gridDim.y batches cover n_docs: c0 < n_docs)
    const uint32_t cols = n_docs - c0 < LABEL_COLS ? n_docs - c0 : LABEL_COLS;
    if (threadIdx.x < cols) {
        const uint64_t first = contig_begin[c0 + threadIdx.x];
        s_first[threadIdx.x] = first;
        s_cnt[threadIdx.x] = (uint32_t)(contig_begin[c0 + threadIdx.x + 1] - first);   // >= 1, checked by the host
        s_at[threadIdx.x] = stage_at[c0 + threadIdx.x];
    }
    __syncthreads();
    for (uint32_t j = 0; j < cols; j++) {                                      // (uniform over the workgroup)
        if (s_at[j] == IN_HBM) continue;
        const int64_t* src = ends + s_first[j];
        int64_t* dst = s_ends + s_at[j];                                        // (s_at + s_cnt <= LABEL_LDS_ENDS, by the host)
        for (uint32_t i = threadIdx.x; i < s_cnt[j]; i += LABEL_BLOCK) dst[i] = src[i];
    }
    __syncthreads();
    const uint64_t tiles = ((uint64_t)n + LABEL_ROWS - 1) / LABEL_ROWS;
    uint32_t missing = 0;
    unsigned long long worst = NO_CELL;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t r0 = t * LABEL_ROWS;
        const uint32_t rows = n - r0 < LABEL_ROWS ? (uint32_t)(n - r0) : LABEL_ROWS;
        const uint32_t items = rows * cols;
        // consecutive work-items take consecutive cells of the batch's stretch of a row, row after row
        for (uint32_t i = threadIdx.x; i < items; i += LABEL_BLOCK) {
            const uint32_t j = i % cols;
            const uint64_t r = r0 + i / cols;
            const uint64_t cell = r * n_docs + c0 + j;
            const int64_t s = off[cell];
            const uint32_t cnt = s_cnt[j], at = s_at[j];
            uint32_t k;
            int64_t left = 0;
            if (at != IN_HBM) {
                const int64_t* e = s_ends + at;
                k = upper_bound(e, cnt, s);
                if (k && k < cnt) left = e[k - 1];
            } else {
                const int64_t* e = ends + s_first[j];
                k = upper_bound(e, cnt, s);
                if (k && k < cnt) left = e[k - 1];
            }
            missing += s == -1 ? 1u : 0u;
            if (k == cnt) {                                                     // at or beyond the total: reported, not labelled
                const unsigned long long where = (row0 + r) * n_docs + c0 + j;
                worst = where < worst ? where : worst;
                contig[cell] = 0;
                rel[cell] = -1;
            } else {
                contig[cell] = k;
                rel[cell] = s - left;
            }
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        missing += __shfl_xor(missing, o, 64);
        const uint32_t lo = __shfl_xor((uint32_t)worst, o, 64), hi = __shfl_xor((uint32_t)(worst >> 32), o, 64);
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
        worst = other < worst ? other : worst;
    }
    if ((threadIdx.x & 63) == 0) {
        if (missing) atomicAdd(absent, (unsigned long long)missing);
        if (worst != NO_CELL) atomicMin(beyond, worst);
    }
}
void lookup(const int64_t* off, uint32_t n, uint32_t n_docs, uint64_t row0, const uint64_t* contig_begin, const int64_t* ends,
            const uint32_t* stage_at, uint32_t* contig, int64_t* rel, uint64_t* beyond, uint64_t* absent, hipStream_t s) {
    if (!n || !n_docs) return;
    const unsigned gy = (n_docs + LABEL_COLS - 1) / LABEL_COLS;
    hipLaunchKernelGGL(k_lookup, dim3(grid_capped(n, LABEL_ROWS, 2048), gy), dim3(LABEL_BLOCK), 0, s, off, n, n_docs, row0,
                       contig_begin, ends, stage_at, contig, rel, reinterpret_cast<unsigned long long*>(beyond),
                       reinterpret_cast<unsigned long long*>(absent));
    MMT_HIP(hipGetLastError());
}

// ---- text -----------------------------------------------------------------------------------------------------------------
// the fourth field: * without blocks, the row's block, or - for none
__device__ __forceinline__ uint32_t block_width(const uint32_t* __restrict__ block, uint64_t r) {
    return !block || block[r] == NO_BLOCK ? 1u : ndigits(block[r]);
}

constexpr uint32_t TEXT_BLOCK = 256, TEXT_WAVES = TEXT_BLOCK / 64;

__global__ __launch_bounds__(TEXT_BLOCK) void k_measure(const uint32_t* __restrict__ len, const int64_t* __restrict__ off,
                                                        const uint32_t* __restrict__ block, const uint32_t* __restrict__ contig,
                                                        const int64_t* __restrict__ rel, uint32_t n, uint32_t n_docs,
                                                        const uint64_t* __restrict__ contig_begin,
                                                        const uint64_t* __restrict__ name_begin, uint64_t* __restrict__ bytes) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * TEXT_WAVES;
    for (uint64_t r = (uint64_t)blockIdx.x * TEXT_WAVES + (threadIdx.x >> 6); r < n; r += stride) {   // (uniform over the wave)
        uint32_t w = 0;
        for (uint32_t d = lane; d < n_docs; d += 64) {
            const uint64_t cell = r * n_docs + d;
            w += int_width(off[cell]) + int_width(rel[cell]);
            if (name_begin) {
                const uint64_t g = contig_begin[d] + contig[cell];
                w += (uint32_t)(name_begin[g + 1] - name_begin[g]);
            } else {
                w += ndigits(contig[cell]);
            }
        }
        w = wave_sum(w);
        // LEN \t starts \t strands \t BLOCK \t contigs \t offsets \n: three fields of N - 1 commas, N strands and theirs
        if (lane == 0)
            bytes[r] = (uint64_t)ndigits(len[r]) + w + 3 * (uint64_t)(n_docs - 1) + (2 * (uint64_t)n_docs - 1) + block_width(block, r) + 6;
    }
}
void measure(const uint32_t* len, const int64_t* off, const uint32_t* block, const uint32_t* contig, const int64_t* rel,
             uint32_t n, uint32_t n_docs, const uint64_t* contig_begin, const uint64_t* name_begin, uint64_t* bytes,
             hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_measure, dim3(grid_capped(n, TEXT_WAVES)), dim3(TEXT_BLOCK), 0, s, len, off, block, contig, rel, n, n_docs,
                       contig_begin, name_begin, bytes);
    MMT_HIP(hipGetLastError());
}

// the names of the row's contigs separated by commas: per 64 cells a prefix sum places the names, then the bytes of the
// stretch are dealt out to the lanes, 64 at a time; a lane finds the cell of its byte by a search among the 64 positions
__device__ __forceinline__ uint32_t put_names(char* t, uint32_t cur, const uint32_t* __restrict__ crow, uint32_t n_docs,
                                              const uint64_t* __restrict__ contig_begin, const uint64_t* __restrict__ name_begin,
                                              const char* __restrict__ names, uint32_t lane) {
    for (uint32_t base = 0; base < n_docs; base += 64) {
        const uint32_t d = base + lane, cnt = n_docs - base < 64 ? n_docs - base : 64;
        uint64_t src = 0; uint32_t nl = 0, wd = 0;
        if (d < n_docs) {
            const uint64_t g = contig_begin[d] + crow[d];
            src = name_begin[g];
            nl = (uint32_t)(name_begin[g + 1] - src);
            wd = nl + (d + 1 < n_docs ? 1 : 0);
        }
        uint32_t total;
        const uint32_t at = wave_excl_sum(wd, lane, total);
        for (uint32_t b0 = 0; b0 < total; b0 += 64) {                          // (uniform over the wave, and so are the shuffles)
            const uint32_t b = b0 + lane;
            uint32_t j = 0;                                                     // the last cell of the 64 that begins at or before b
#pragma unroll
            for (uint32_t step = 32; step; step >>= 1) {
                const uint32_t cand = j + step;
                const uint32_t a = __shfl(at, (int)(cand & 63), 64);
                if (cand < cnt && a <= b) j = cand;
            }
            const uint32_t aj = __shfl(at, (int)j, 64), nlj = __shfl(nl, (int)j, 64);
            const uint32_t slo = __shfl((uint32_t)src, (int)j, 64), shi = __shfl((uint32_t)(src >> 32), (int)j, 64);
            if (b < total) {
                const uint32_t o = b - aj;
                t[cur + b] = o < nlj ? names[(((uint64_t)shi << 32) | slo) + o] : ',';
            }
        }
        cur += total;
    }
    return cur;
}

__global__ __launch_bounds__(TEXT_BLOCK) void k_write_lines(const uint32_t* __restrict__ len, const int64_t* __restrict__ off,
                                                            const uint8_t* __restrict__ st, const uint32_t* __restrict__ block,
                                                            const uint32_t* __restrict__ contig, const int64_t* __restrict__ rel,
                                                            uint32_t n, uint32_t n_docs, const uint64_t* __restrict__ contig_begin,
                                                            const uint64_t* __restrict__ name_begin, const char* __restrict__ names,
                                                            const uint64_t* __restrict__ text_off, uint64_t text_base,
                                                            char* __restrict__ text) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * TEXT_WAVES;
    for (uint64_t r = (uint64_t)blockIdx.x * TEXT_WAVES + (threadIdx.x >> 6); r < n; r += stride) {   // (uniform over the wave)
        char* t = text + (text_off[r] - text_base);
        const uint32_t nl = ndigits(len[r]);
        if (lane == 0) { put_uint(t, len[r], nl); t[nl] = '\t'; }
        uint32_t cur = put_numbers(t, nl + 1, off + r * n_docs, n_docs, lane);
        if (lane == 0) t[cur] = '\t';
        cur = put_strands(t, cur + 1, st + r * n_docs, n_docs, lane);
        const uint32_t bw = block_width(block, r);
        if (lane == 0) {
            t[cur] = '\t';
            if (!block) t[cur + 1] = '*';
            else if (block[r] == NO_BLOCK) t[cur + 1] = '-';
            else put_uint(t + cur + 1, block[r], bw);
            t[cur + 1 + bw] = '\t';
        }
        cur += bw + 2;
        cur = name_begin ? put_names(t, cur, contig + r * n_docs, n_docs, contig_begin, name_begin, names, lane)
                         : put_numbers(t, cur, contig + r * n_docs, n_docs, lane);
        if (lane == 0) t[cur] = '\t';
        cur = put_numbers(t, cur + 1, rel + r * n_docs, n_docs, lane);
        if (lane == 0) t[cur] = '\n';
    }
}
void write_lines(const uint32_t* len, const int64_t* off, const uint8_t* st, const uint32_t* block, const uint32_t* contig,
                 const int64_t* rel, uint32_t n, uint32_t n_docs, const uint64_t* contig_begin, const uint64_t* name_begin,
                 const char* names, const uint64_t* text_off, uint64_t text_base, char* text, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_write_lines, dim3(grid_capped(n, TEXT_WAVES)), dim3(TEXT_BLOCK), 0, s, len, off, st, block, contig, rel, n,
                       n_docs, contig_begin, name_begin, names, text_off, text_base, text);
    MMT_HIP(hipGetLastError());
}

}}  // namespace mmt::lk
