// bed_kernels.hip -- see bed_kernels.hpp.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bed_kernels.hpp"
#include "device_utils.hpp"
#include "launch_grid.hpp"
#include "table_text.hpp"

namespace mmt { namespace bk {

using namespace tt;      // the decimals and the contig search

// ---- select ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SELECT_BLOCK) void k_select_flags(const int64_t* __restrict__ off, const uint32_t* __restrict__ length,
                                                               const uint32_t* __restrict__ row_block,
                                                               const uint32_t* __restrict__ blocks, uint32_t n, uint32_t n_docs,
                                                               uint32_t col, int64_t min_single, uint32_t* __restrict__ flag,
                                                               uint32_t* __restrict__ present) {
    const uint64_t tiles = ((uint64_t)n + SELECT_TILE - 1) / SELECT_TILE;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
#pragma unroll
        for (uint32_t q = 0; q < SELECT_ITEMS; q++) {             // coalesced: consecutive work-items take consecutive rows
            const uint64_t r = t * SELECT_TILE + (uint64_t)q * SELECT_BLOCK + threadIdx.x;
            if (r >= n) continue;
            const bool long_enough = (int64_t)length[r] >= min_single;
            if (row_block) {
                const uint32_t b = row_block[r];
                flag[r] = (b == NO_BLOCK ? long_enough : blocks[2 * (uint64_t)b] == (uint32_t)r) ? 1u : 0u;
            } else {
                const bool here = off[r * n_docs + col] != -1;
                present[r] = here ? 1u : 0u;
                flag[r] = (here && long_enough) ? 1u : 0u;
            }
        }
    }
}
void select_flags(const int64_t* off, const uint32_t* length, const uint32_t* row_block, const uint32_t* blocks, uint32_t n,
                  uint32_t n_docs, uint32_t col, int64_t min_single, uint32_t* flag, uint32_t* present, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_select_flags, dim3(grid_capped(n, SELECT_TILE)), dim3(SELECT_BLOCK), 0, s, off, length, row_block, blocks,
                       n, n_docs, col, min_single, flag, present);
    MMT_HIP(hipGetLastError());
}

__global__ void k_list_records(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ number,
                               const uint32_t* __restrict__ rank, const uint32_t* __restrict__ row_block,
                               const uint32_t* __restrict__ blocks, uint32_t n, uint32_t* __restrict__ rows,
                               int64_t* __restrict__ name) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
        if (!flag[r]) continue;
        const uint64_t k = number[r];
        const uint32_t b = row_block ? row_block[r] : NO_BLOCK;
        rows[2 * k] = (uint32_t)r;
        rows[2 * k + 1] = b == NO_BLOCK ? (uint32_t)r : blocks[2 * (uint64_t)b + 1];
        name[k] = b == NO_BLOCK ? -1 - (int64_t)(rank ? rank[r] : (uint32_t)r) : (int64_t)b;
    }
}
void list_records(const uint32_t* flag, const uint32_t* number, const uint32_t* rank, const uint32_t* row_block,
                  const uint32_t* blocks, uint32_t n, uint32_t* rows, int64_t* name, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_list_records, dim3(grid_capped(n, 256)), dim3(256), 0, s, flag, number, rank, row_block, blocks, n, rows,
                       name);
    MMT_HIP(hipGetLastError());
}

// ---- gather ---------------------------------------------------------------------------------------------------------------
// The tile of inversion_kernels.hip's head gather: TR records x TC columns.  Read: the 32 lanes of a half-wave take 32
// consecutive cells of the record's first row and of its last row (256 contiguous bytes each), 8 records per step.  Write: a
// wave takes 64 consecutive records of one column.  The LDS tiles are [column][record] with one entry of padding per column.
constexpr uint32_t TR = 64, TC = 32;

__global__ __launch_bounds__(256) void k_gather(const int64_t* __restrict__ off, const uint8_t* __restrict__ st,
                                                const uint32_t* __restrict__ length, const uint32_t* __restrict__ rows,
                                                uint32_t n_rec, uint32_t n_docs, uint32_t c0, uint32_t n_cols,
                                                int64_t* __restrict__ begin, int64_t* __restrict__ end,
                                                uint8_t* __restrict__ strand) {
    __shared__ int64_t tile_b[TC][TR + 1];
    __shared__ int64_t tile_e[TC][TR + 1];
    __shared__ uint8_t tile_s[TC][TR + 4];
    const uint32_t tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t cb = blockIdx.y * TC;
    const uint32_t tiles = (uint32_t)(((uint64_t)n_rec + TR - 1) / TR);
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t k0 = (uint64_t)t * TR;
        for (uint32_t i = ty; i < TR; i += 8) {
            const uint64_t k = k0 + i;
            if (k < n_rec && cb + tx < n_cols) {
                const uint64_t first = rows[2 * k], last = rows[2 * k + 1];
                const uint64_t cell_l = last * n_docs + c0 + cb + tx;
                const int64_t s_last = off[cell_l];
                const uint8_t plus = st[cell_l] ? 1 : 0;
                int64_t s_first = s_last;
                if (first != last) s_first = off[first * n_docs + c0 + cb + tx];
                tile_b[tx][i] = plus ? s_first : s_last;
                tile_e[tx][i] = plus ? s_last + (int64_t)length[last] : s_first + (int64_t)length[first];
                tile_s[tx][i] = plus;
            }
        }
        __syncthreads();
        for (uint32_t c = wave; c < TC; c += 4) {
            if (cb + c >= n_cols) break;                     // (uniform over the wave)
            const uint64_t k = k0 + lane;
            if (k < n_rec) {
                const uint64_t at = (uint64_t)(cb + c) * n_rec + k;
                begin[at] = tile_b[c][lane];
                end[at] = tile_e[c][lane];
                strand[at] = tile_s[c][lane];
            }
        }
        __syncthreads();
    }
}
void gather(const int64_t* off, const uint8_t* st, const uint32_t* length, const uint32_t* rows, uint32_t n_rec, uint32_t n_docs,
            uint32_t c0, uint32_t n_cols, int64_t* begin, int64_t* end, uint8_t* strand, hipStream_t s) {
    if (!n_rec || !n_cols) return;
    const uint64_t tiles = ((uint64_t)n_rec + TR - 1) / TR;
    const unsigned gx = (unsigned)(tiles < (1u << 18) ? tiles : (1u << 18)), gy = (n_cols + TC - 1) / TC;
    hipLaunchKernelGGL(k_gather, dim3(gx, gy), dim3(256), 0, s, off, st, length, rows, n_rec, n_docs, c0, n_cols, begin, end,
                       strand);
    MMT_HIP(hipGetLastError());
}

// ---- contig lookup --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lookup(const int64_t* __restrict__ begin, const int64_t* __restrict__ end,
                                                const uint8_t* __restrict__ strand, const int64_t* __restrict__ name,
                                                uint32_t n_rec, uint32_t c0, uint32_t n_cols,
                                                const uint64_t* __restrict__ contig_begin, const int64_t* __restrict__ ends,
                                                int64_t* __restrict__ records, unsigned long long* __restrict__ clamped) {
    __shared__ int64_t s_ends[BED_LDS_CONTIGS];
    uint32_t beyond = 0;
    for (uint32_t j = blockIdx.y; j < n_cols; j += gridDim.y) {               // (uniform over the workgroup)
        const uint64_t cfirst = contig_begin[c0 + j];
        const uint32_t cnt = (uint32_t)(contig_begin[c0 + j + 1] - cfirst);   // >= 1, checked by the host
        const int64_t* col_ends = ends + cfirst;
        const bool staged = cnt <= BED_LDS_CONTIGS;
        if (staged) {
            __syncthreads();                                                  // (the column before is done with s_ends)
            for (uint32_t i = threadIdx.x; i < cnt; i += blockDim.x) s_ends[i] = col_ends[i];
            __syncthreads();
        }
        const int64_t* search = staged ? s_ends : col_ends;
        const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
        for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_rec; k += stride) {
            const uint64_t at = (uint64_t)j * n_rec + k;
            const int64_t b = begin[at];
            uint32_t i = upper_bound(search, cnt, b);
            if (i == cnt) { i = cnt - 1; beyond++; }
            const int64_t rel = b - (i ? search[i - 1] : 0);
            int64_t* out = records + at * RECORD_FIELDS;
            out[0] = (int64_t)i;
            out[1] = rel;
            out[2] = rel + (end[at] - b);
            out[3] = name[k];
            out[4] = (int64_t)strand[at];
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) beyond += __shfl_xor(beyond, o, 64);
    if ((threadIdx.x & 63) == 0 && beyond) atomicAdd(clamped, (unsigned long long)beyond);
}
void lookup(const int64_t* begin, const int64_t* end, const uint8_t* strand, const int64_t* name, uint32_t n_rec, uint32_t c0,
            uint32_t n_cols, const uint64_t* contig_begin, const int64_t* ends, int64_t* records, uint64_t* clamped, hipStream_t s) {
    if (!n_rec || !n_cols) return;
    hipLaunchKernelGGL(k_lookup, dim3(grid_capped(n_rec, 256, 2048), n_cols < 1024 ? n_cols : 1024), dim3(256), 0, s, begin, end,
                       strand, name, n_rec, c0, n_cols, contig_begin, ends, records, reinterpret_cast<unsigned long long*>(clamped));
    MMT_HIP(hipGetLastError());
}

// ---- text -----------------------------------------------------------------------------------------------------------------
// block_<b> for name >= 0, mum_<i> for name = -1 - i
__device__ __forceinline__ uint32_t label_width(int64_t name) {
    return name >= 0 ? 6 + ndigits((uint64_t)name) : 4 + ndigits((uint64_t)(-1 - name));
}

__global__ void k_measure(const int64_t* __restrict__ records, uint32_t n_rec, const uint64_t* __restrict__ name_begin,
                          uint64_t first_contig, uint32_t* __restrict__ bytes) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_rec; k += stride) {
        const int64_t* rec = records + k * RECORD_FIELDS;
        const uint64_t g = first_contig + (uint64_t)rec[0];
        bytes[k] = (uint32_t)(name_begin[g + 1] - name_begin[g]) + int_width(rec[1]) + int_width(rec[2]) + label_width(rec[3]) + 6;
    }
}
void measure(const int64_t* records, uint32_t n_rec, const uint64_t* name_begin, uint64_t first_contig, uint32_t* bytes,
             hipStream_t s) {
    if (!n_rec) return;
    hipLaunchKernelGGL(k_measure, dim3(grid_capped(n_rec, 256)), dim3(256), 0, s, records, n_rec, name_begin, first_contig, bytes);
    MMT_HIP(hipGetLastError());
}

// one line; dst is LDS or HBM
__device__ __forceinline__ void put_line(char* dst, const int64_t* rec, const uint64_t* __restrict__ name_begin,
                                         const char* __restrict__ names, uint64_t first_contig) {
    const uint64_t g = first_contig + (uint64_t)rec[0];
    const uint64_t a = name_begin[g], b = name_begin[g + 1];
    for (uint64_t i = a; i < b; i++) *dst++ = names[i];
    *dst++ = '\t';
    dst = put_int(dst, rec[1]);
    *dst++ = '\t';
    dst = put_int(dst, rec[2]);
    *dst++ = '\t';
    const int64_t name = rec[3];
    if (name >= 0) {
        dst[0] = 'b'; dst[1] = 'l'; dst[2] = 'o'; dst[3] = 'c'; dst[4] = 'k'; dst[5] = '_';
        dst = put_uint(dst + 6, (uint64_t)name, ndigits((uint64_t)name));
    } else {
        const uint64_t i = (uint64_t)(-1 - name);
        dst[0] = 'm'; dst[1] = 'u'; dst[2] = 'm'; dst[3] = '_';
        dst = put_uint(dst + 4, i, ndigits(i));
    }
    dst[0] = '\t';
    dst[1] = rec[4] ? '+' : '-';
    dst[2] = '\n';
}

constexpr uint32_t WRITE_WAVES = 4, WRITE_CHUNK = WRITE_WAVES * BED_WAVE_RECORDS;
constexpr uint32_t STAGE_DWORDS = BED_LDS_BYTES / 4 + 2;     // (the word assembly reads up to two dwords past the span)

__global__ __launch_bounds__(WRITE_WAVES * 64) void k_write_lines(const int64_t* __restrict__ records, uint32_t n_rec,
                                                                  const uint64_t* __restrict__ name_begin,
                                                                  const char* __restrict__ names, uint64_t first_contig,
                                                                  const uint64_t* __restrict__ offset, uint64_t base,
                                                                  char* __restrict__ text) {
    __shared__ uint32_t stage[WRITE_WAVES][STAGE_DWORDS];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t chunks = ((uint64_t)n_rec + WRITE_CHUNK - 1) / WRITE_CHUNK;
    char* lds = reinterpret_cast<char*>(stage[wave]);
    for (uint64_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {            // (uniform over the workgroup)
        const uint64_t k0 = ch * WRITE_CHUNK + (uint64_t)wave * BED_WAVE_RECORDS;
        const bool active = k0 < n_rec;                                        // (uniform over the wave, like all below but k)
        const uint64_t k1 = active ? (k0 + BED_WAVE_RECORDS < n_rec ? k0 + BED_WAVE_RECORDS : n_rec) : k0;
        const uint64_t o0 = active ? offset[k0] : 0, o1 = active ? offset[k1] : 0;
        const uint64_t span = o1 - o0;
        const bool staged = active && span <= BED_LDS_BYTES;
        const uint64_t k = k0 + lane;
        if (active && k < k1) {
            const uint64_t mine = offset[k];
            put_line(staged ? lds + (mine - o0) : text + (mine - base), records + k * RECORD_FIELDS, name_begin, names, first_contig);
        }
        __syncthreads();
        if (staged) {
            char* out = text + (o0 - base);
            const uint32_t n = (uint32_t)span;
            uint32_t head = (uint32_t)((8 - (reinterpret_cast<uintptr_t>(out) & 7)) & 7);
            if (head > n) head = n;
            const uint32_t words = (n - head) >> 3, tail = head + (words << 3);
            if (lane < head) out[lane] = lds[lane];
            uint64_t* out8 = reinterpret_cast<uint64_t*>(out + head);
            for (uint32_t w = lane; w < words; w += 64) {
                const uint32_t at = head + (w << 3), sh = (at & 3) * 8;
                const uint32_t* p = stage[wave] + (at >> 2);
                const uint32_t a = p[0], b = p[1], c = p[2];
                const uint32_t lo = sh ? (a >> sh) | (b << (32 - sh)) : a;
                const uint32_t hi = sh ? (b >> sh) | (c << (32 - sh)) : b;
                out8[w] = (uint64_t)lo | ((uint64_t)hi << 32);
            }
            if (tail + lane < n) out[tail + lane] = lds[tail + lane];          // (fewer than 8 bytes)
        }
        __syncthreads();                                                       // the next chunk writes the stage again
    }
}
void write_lines(const int64_t* records, uint32_t n_rec, const uint64_t* name_begin, const char* names, uint64_t first_contig,
                 const uint64_t* offset, uint64_t base, char* text, hipStream_t s) {
    if (!n_rec) return;
    hipLaunchKernelGGL(k_write_lines, dim3(grid_capped(n_rec, WRITE_CHUNK)), dim3(WRITE_WAVES * 64), 0, s, records, n_rec,
                       name_begin, names, first_contig, offset, base, text);
    MMT_HIP(hipGetLastError());
}

}}  // namespace mmt::bk
