// sequence_kernels.hip -- see sequence_kernels.hpp.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sequence_kernels.hpp"
#include "device_utils.hpp"
#include "launch_grid.hpp"
#include "table_text.hpp"

namespace mmt { namespace sq {

using namespace tt;      // the decimals, the search

// ---- 16 bytes in two register pairs: byte i of the chunk in bits [8 i, 8 i + 8) ------------------------------------------------
struct B16 { uint64_t lo, hi; };

__device__ __forceinline__ B16 or16(B16 a, B16 b) { return B16{a.lo | b.lo, a.hi | b.hi}; }
// bytes [s, 16) of x at [0, 16 - s), s in [0, 16]
__device__ __forceinline__ B16 shr_bytes(B16 x, uint32_t s) {
    const uint32_t bits = 8 * s;
    if (bits == 0) return x;
    if (bits >= 128) return B16{0, 0};
    if (bits >= 64) return B16{x.hi >> (bits - 64), 0};
    return B16{(x.lo >> bits) | (x.hi << (64 - bits)), x.hi >> bits};
}
// bytes [0, 16 - s) of x at [s, 16), s in [0, 16]
__device__ __forceinline__ B16 shl_bytes(B16 x, uint32_t s) {
    const uint32_t bits = 8 * s;
    if (bits == 0) return x;
    if (bits >= 128) return B16{0, 0};
    if (bits >= 64) return B16{0, x.lo << (bits - 64)};
    return B16{x.lo << bits, (x.hi << bits) | (x.lo >> (64 - bits))};
}
// the first n bytes of x, n in [0, 16]
__device__ __forceinline__ B16 low_bytes(B16 x, uint32_t n) {
    if (n >= 16) return x;
    if (n >= 8) return B16{x.lo, n == 8 ? 0 : x.hi & (~0ull >> (8 * (16 - n)))};
    return B16{n == 0 ? 0 : x.lo & (~0ull >> (8 * (8 - n))), 0};
}
__device__ __forceinline__ uint64_t bswap8(uint64_t x) { return __builtin_bswap64(x); }
__device__ __forceinline__ B16 reverse16(B16 x) { return B16{bswap8(x.hi), bswap8(x.lo)}; }

// a-z -> A-Z in every byte; bytes of 0x80 and above stay
__device__ __forceinline__ uint64_t upper8(uint64_t x) {
    const uint64_t H = 0x8080808080808080ull, x7 = x & ~H;
    const uint64_t ge_a = x7 + 0x1f1f1f1f1f1f1f1full;        // bit 7 of a byte: x7 >= 0x61
    const uint64_t gt_z = x7 + 0x0505050505050505ull;        //                  x7 >= 0x7b
    const uint64_t lower = ge_a & ~gt_z & ~x & H;
    return x - (lower >> 2);
}
// 0x01 in every byte of x that equals v (v < 0x80)
__device__ __forceinline__ uint64_t eq8(uint64_t x, uint32_t v) {
    const uint64_t H = 0x8080808080808080ull, y = x ^ (0x0101010101010101ull * v);
    return (~(((y & ~H) + ~H) | y) & H) >> 7;
}
// The complement of a base.  The reference's Python tool leaves this to Biopython, which these machines do not have, so the
// table is decided here (and mirrored by tests/seqmodel.py): A<->T, C<->G, M<->K, R<->Y, V<->B, H<->D; W, S, N, X and every
// other byte -- lower case included -- are copied unchanged.  A pair (a, b) is exchanged by XOR with a ^ b.
__device__ __forceinline__ uint64_t complement8(uint64_t x) {
    uint64_t flip = 0;
    flip |= (eq8(x, 'A') | eq8(x, 'T')) * ('A' ^ 'T');
    flip |= (eq8(x, 'C') | eq8(x, 'G')) * ('C' ^ 'G');
    flip |= (eq8(x, 'M') | eq8(x, 'K')) * ('M' ^ 'K');
    flip |= (eq8(x, 'R') | eq8(x, 'Y')) * ('R' ^ 'Y');
    flip |= (eq8(x, 'V') | eq8(x, 'B')) * ('V' ^ 'B');
    flip |= (eq8(x, 'H') | eq8(x, 'D')) * ('H' ^ 'D');
    return x ^ flip;
}

// text positions [p, p + 16) as they lie behind one another in V: two aligned reads, shifted (p < T.n; the padding behind
// the text of either layout covers the second read)
__device__ __forceinline__ B16 load16(const TextRef& T, uint64_t p0) {
    const uint4 v = tx_load16(T, p0);
    return B16{(uint64_t)v.x | ((uint64_t)v.y << 32), (uint64_t)v.z | ((uint64_t)v.w << 32)};
}
__device__ __forceinline__ B16 fetch16(const TextRef& T, uint64_t p) {
    const uint64_t p0 = p & ~15ull;
    const uint32_t s = (uint32_t)(p & 15);
    const B16 a = load16(T, p0);
    if (!s) return a;
    const B16 b = load16(T, p0 + 16);
    return or16(shr_bytes(a, s), shl_bytes(b, 16 - s));
}

// `>mum_<k>\n`: 6 + ndigits(k) bytes, at most 16
__device__ __forceinline__ B16 header16(uint32_t k) {
    B16 h{'\n', 0};
    do { h = shl_bytes(h, 1); h.lo |= (uint64_t)('0' + k % 10); k /= 10; } while (k);
    h = shl_bytes(h, 5);
    h.lo |= 0x5f6d756d3eull;                                  // ">mum_", '>' in the first byte
    return h;
}

// bytes [j, j + take) of the bases of a record (take in [1, 16]) in the first bytes of the result; what lies behind them is
// not defined
__device__ __forceinline__ B16 bases16(const TextRef& T, uint64_t source, uint64_t nb, uint64_t j, uint32_t take, Format f) {
    const bool rev = (source & REVERSE) != 0;
    const uint64_t s = source & ~REVERSE;
    B16 x;
    if (!rev) x = fetch16(T, s + j);
    else x = shr_bytes(reverse16(fetch16(T, s + nb - j - take)), 16 - take);      // the range read backwards
    if (f.upper) { x.lo = upper8(x.lo); x.hi = upper8(x.hi); }
    if (rev) { x.lo = complement8(x.lo); x.hi = complement8(x.hi); }
    return x;
}

// the `want` bytes of the text from byte q of record k on (k < k1: the records behind k follow where it ends)
__device__ __forceinline__ B16 assemble(const TextRef& T, const uint64_t* __restrict__ source, const uint32_t* __restrict__ bases,
                                        uint32_t k, uint32_t k1, uint32_t n, uint64_t q, uint32_t want, Format f) {
    B16 out{0, 0};
    uint32_t b = 0;
    while (b < want && k < k1) {
        const uint64_t hdr = 6 + ndigits(k), nb = bases[k];
        if (q < hdr) {
            const uint32_t take = hdr - q < CHUNK - b ? (uint32_t)(hdr - q) : CHUNK - b;
            out = or16(out, shl_bytes(low_bytes(shr_bytes(header16(k), (uint32_t)q), take), b));
            b += take; q += take;
        }
        if (b < CHUNK && q >= hdr && q < hdr + nb) {
            const uint64_t j = q - hdr;
            const uint32_t take = nb - j < CHUNK - b ? (uint32_t)(nb - j) : CHUNK - b;
            out = or16(out, shl_bytes(low_bytes(bases16(T, source[k], nb, j, take, f), take), b));
            b += take; q += take;
        }
        uint64_t end = hdr + nb;
        if (f.terminator) {
            if (b < CHUNK && q == end) { out = or16(out, shl_bytes(B16{'#', 0}, b)); b++; q++; }
            end++;
        }
        if (!f.join || k + 1 < n) {
            if (b < CHUNK && q == end) { out = or16(out, shl_bytes(B16{'\n', 0}, b)); b++; q++; }
            end++;
        }
        if (b < CHUNK) { k++; q = 0; }                        // (q == end: the record is complete)
    }
    return out;
}

// ---- measure ---------------------------------------------------------------------------------------------------------------
__global__ void k_clear_flags(uint64_t* __restrict__ flags) {
    if (threadIdx.x < N_FLAGS) flags[threadIdx.x] = threadIdx.x <= BEYOND ? NO_ROW : 0;
}
void clear_flags(uint64_t* flags, hipStream_t s) {
    hipLaunchKernelGGL(k_clear_flags, dim3(1), dim3(64), 0, s, flags);
    MMT_HIP(hipGetLastError());
}

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void k_measure(const int64_t* __restrict__ off, const uint8_t* __restrict__ strands,
                                                 const uint32_t* __restrict__ length, uint32_t n, uint32_t n_docs, uint32_t col,
                                                 uint64_t doc_begin, uint64_t doc_len, Format f, uint64_t* __restrict__ bytes,
                                                 uint64_t* __restrict__ source, uint32_t* __restrict__ bases,
                                                 unsigned long long* __restrict__ flags) {
    unsigned long long written = 0, clipped = 0, empty = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
        const uint64_t cell = k * n_docs + col;
        const int64_t s = off[cell];
        const uint32_t len = length[k];
        uint32_t nb = 0;
        if (s < -1) atomicMin(flags + BAD_START, (unsigned long long)k);
        else if (s == -1) { if (!f.lenient) atomicMin(flags + PARTIAL, (unsigned long long)k); }
        else if ((uint64_t)s > doc_len) { if (!f.lenient) atomicMin(flags + BEYOND, (unsigned long long)k); }
        else {
            const uint64_t room = doc_len - (uint64_t)s;
            nb = len < room ? len : (uint32_t)room;
            if (nb < len) clipped++;
        }
        if (!nb) empty++;
        written += nb;
        const bool rev = f.strands && !strands[cell];
        source[k] = (nb ? doc_begin + (uint64_t)s : 0) | (rev ? REVERSE : 0);
        bases[k] = nb;
        bytes[k] = 6ull + ndigits(k) + nb + (f.terminator ? 1 : 0) + ((!f.join || k + 1 < n) ? 1 : 0);
    }
    written = wave_sum64(written); clipped = wave_sum64(clipped); empty = wave_sum64(empty);
    if ((threadIdx.x & 63) == 0) {
        if (written) atomicAdd(flags + BASES, written);
        if (clipped) atomicAdd(flags + CLIPPED, clipped);
        if (empty) atomicAdd(flags + EMPTY, empty);
    }
}
void measure(const int64_t* off, const uint8_t* strands, const uint32_t* length, uint32_t n, uint32_t n_docs, uint32_t col,
             uint64_t doc_begin, uint64_t doc_len, Format f, uint64_t* bytes, uint64_t* source, uint32_t* bases, uint64_t* flags,
             hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_measure, dim3(grid_capped(n, 256, 2048)), dim3(256), 0, s, off, strands, length, n, n_docs, col, doc_begin,
                       doc_len, f, bytes, source, bases, reinterpret_cast<unsigned long long*>(flags));
    MMT_HIP(hipGetLastError());
}

// ---- format ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FORMAT_BLOCK) void k_format(TextRef T, const uint64_t* __restrict__ offset,
                                                         const uint64_t* __restrict__ source, const uint32_t* __restrict__ bases,
                                                         uint32_t k0, uint32_t k1, uint32_t n, uint64_t base, Format f, char* __restrict__ dst) {
    __shared__ uint64_t s_off[LDS_RECORDS];
    __shared__ uint32_t s_range[2];
    const uint64_t bytes = offset[k1] - base;                // of the piece: offset[k0] = base
    const uint64_t chunks = (bytes + CHUNK - 1) / CHUNK;     // (the last one may be cut short)
    const uint64_t tiles = (chunks + TILE_CHUNKS - 1) / TILE_CHUNKS;
    const uint64_t* piece = offset + k0;                    // offsets of the piece's records: piece[0] = base
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {               // (uniform over the workgroup)
        const uint64_t c0 = t * TILE_CHUNKS, c1 = c0 + TILE_CHUNKS < chunks ? c0 + TILE_CHUNKS : chunks;
        // the records of the tile's first and last byte
        if (threadIdx.x < 2) {
            const uint64_t at = base + (threadIdx.x ? (c1 * CHUNK < bytes ? c1 * CHUNK : bytes) - 1 : c0 * CHUNK);
            s_range[threadIdx.x] = last_at_or_before(k1 - k0, at, [&](uint32_t i) { return piece[i]; });
        }
        __syncthreads();
        const uint32_t r_lo = s_range[0], cnt = s_range[1] - r_lo + 1;
        const bool staged = cnt <= LDS_RECORDS;
        if (staged)
            for (uint32_t i = threadIdx.x; i < cnt; i += FORMAT_BLOCK) s_off[i] = piece[r_lo + i];
        __syncthreads();
#pragma unroll 1
        for (uint32_t it = 0; it < FORMAT_ITEMS; it++) {      // coalesced: consecutive lanes store consecutive chunks
            const uint64_t c = c0 + (uint64_t)it * FORMAT_BLOCK + threadIdx.x;
            if (c >= c1) continue;
            const uint64_t at = base + c * CHUNK;
            uint32_t r;
            uint64_t begin;
            if (staged) {
                r = last_at_or_before(cnt, at, [&](uint32_t i) { return s_off[i]; });
                begin = s_off[r];
            } else {
                r = last_at_or_before(cnt, at, [&](uint32_t i) { return piece[r_lo + i]; });
                begin = piece[r_lo + r];
            }
            const B16 v = assemble(T, source, bases, k0 + r_lo + r, k1, n, at - begin, CHUNK, f);
            if ((c + 1) * CHUNK <= bytes) {
                uint4 w;
                w.x = (uint32_t)v.lo; w.y = (uint32_t)(v.lo >> 32); w.z = (uint32_t)v.hi; w.w = (uint32_t)(v.hi >> 32);
                reinterpret_cast<uint4*>(dst)[c] = w;
            } else {                                           // the bytes behind the last whole chunk, one by one
                const uint32_t rest = (uint32_t)(bytes - c * CHUNK);
                for (uint32_t i = 0; i < rest; i++) dst[c * CHUNK + i] = (char)(shr_bytes(v, i).lo & 0xff);
            }
        }
        __syncthreads();                                      // the next tile stages its offsets
    }
}
void format(const TextRef& T, const uint64_t* offset, const uint64_t* source, const uint32_t* bases, uint32_t k0, uint32_t k1,
            uint32_t n, uint64_t base, uint64_t bytes_at_most, Format f, char* dst, hipStream_t s) {
    if (k0 >= k1 || !bytes_at_most) return;
    const uint64_t tiles = ((bytes_at_most + CHUNK - 1) / CHUNK + TILE_CHUNKS - 1) / TILE_CHUNKS;
    hipLaunchKernelGGL(k_format, dim3(grid_capped(tiles, 1, 1u << 16)), dim3(FORMAT_BLOCK), 0, s, T, offset, source, bases, k0, k1, n,
                       base, f, dst);
    MMT_HIP(hipGetLastError());
}

}}  // namespace mmt::sq
