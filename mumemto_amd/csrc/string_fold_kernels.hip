// string_fold_kernels.hip -- see string_fold_kernels.hpp.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_utils.hpp"
#include "launch_grid.hpp"
#include "string_fold_kernels.hpp"
#include "table_text.hpp"

namespace mmt { namespace sk {

using tt::last_at_or_before;
using tt::upper_bound;   // the `#` at or beyond x is the first record end beyond x: one search serves both

// ---- the tables as they arrive ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_check_table(const uint32_t* __restrict__ len, const int64_t* __restrict__ starts, uint32_t n,
                                                     uint32_t n_cols, PartState* __restrict__ state) {
    const uint64_t cells = (uint64_t)n * n_cols, stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t bad = 0;
    unsigned long long sum = 0;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < cells; t += stride) {
        const int64_t v = starts[t];
        if (v == -1) bad |= PART_ABSENT;
        if (t % n_cols == 0) {
            if (t && starts[t - n_cols] > v) bad |= PART_UNSORTED;
            if (len) sum += (unsigned long long)len[t / n_cols] + 1;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        bad |= __shfl_xor(bad, o, 64);
        const uint32_t lo = __shfl_xor((uint32_t)sum, o, 64), hi = __shfl_xor((uint32_t)(sum >> 32), o, 64);
        sum += ((unsigned long long)hi << 32) | lo;
    }
    if ((threadIdx.x & 63) == 0) {
        if (bad) atomicOr(&state->flags, bad);
        if (sum) atomicAdd(&state->positions, sum);
    }
}
void check_table(const uint32_t* len, const int64_t* starts, uint32_t n, uint32_t n_cols, PartState* state, hipStream_t s) {
    if (!n || !n_cols) return;
    hipLaunchKernelGGL(k_check_table, dim3(grid_capped((uint64_t)n * n_cols, 256, 2048)), dim3(256), 0, s, len, starts, n, n_cols, state);
    MMT_HIP(hipGetLastError());
}

// ---- split ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_count_pieces(const uint32_t* __restrict__ mom_len, const int64_t* __restrict__ mom_starts,
                                                      uint32_t m, uint32_t S, const int64_t* __restrict__ rec_end0, uint32_t n_rec0,
                                                      uint32_t* __restrict__ first, uint32_t* __restrict__ pieces) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= m) return;
    const int64_t s0 = mom_starts[(uint64_t)r * S];
    const uint32_t a = upper_bound(rec_end0, n_rec0, s0), b = upper_bound(rec_end0, n_rec0, s0 + (int64_t)mom_len[r]);
    first[r] = a;
    pieces[r] = b - a + 1;                       // (s0 <= s0 + L: b >= a)
}
void count_pieces(const uint32_t* mom_len, const int64_t* mom_starts, uint32_t m, uint32_t S, const int64_t* rec_end0, uint32_t n_rec0,
                  uint32_t* first, uint32_t* pieces, hipStream_t s) {
    if (!m) return;
    hipLaunchKernelGGL(k_count_pieces, dim3(grid_for(m, 256)), dim3(256), 0, s, mom_len, mom_starts, m, S, rec_end0, n_rec0, first,
                       pieces);
    MMT_HIP(hipGetLastError());
}

__global__ __launch_bounds__(256) void k_cut_pieces(const uint32_t* __restrict__ mom_len, const int64_t* __restrict__ mom_starts,
                                                    const uint8_t* __restrict__ mom_strands, uint32_t m, uint32_t S,
                                                    const int64_t* __restrict__ rec_end0, uint32_t n_rec0,
                                                    const uint32_t* __restrict__ first, const uint64_t* __restrict__ piece_begin,
                                                    uint32_t n_pieces, uint32_t* __restrict__ piece_row, int64_t* __restrict__ seg_len,
                                                    int64_t* __restrict__ seg_start, uint8_t* __restrict__ keep) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pieces) return;
    // the last row whose pieces begin at or before p (every row has a piece)
    const uint32_t r = last_at_or_before(m, p, [&](uint32_t i) { return piece_begin[i]; });
    const uint32_t k = p - (uint32_t)piece_begin[r], cnt = (uint32_t)(piece_begin[r + 1] - piece_begin[r]), a = first[r];
    const int64_t L = (int64_t)mom_len[r], s0 = mom_starts[(uint64_t)r * S];
    const int64_t left = k == 0 ? 0 : rec_end0[a + k - 1] - 1 - s0 + 1;             // (a + k - 1 < a + cnt - 1 <= n_rec0)
    const int64_t end = k == cnt - 1 ? L : rec_end0[a + k] - 1 - s0;
    const int64_t nl = end - left;
    piece_row[p] = r;
    seg_len[p] = nl;
    keep[p] = nl >= (int64_t)MIN_SEGMENT || cnt == 1 ? 1 : 0;
    for (uint32_t i = 0; i < S; i++) {
        const uint64_t cell = (uint64_t)r * S + i;
        seg_start[(uint64_t)p * S + i] = mom_starts[cell] + (mom_strands[cell] ? left : L - end);
    }
}
void cut_pieces(const uint32_t* mom_len, const int64_t* mom_starts, const uint8_t* mom_strands, uint32_t m, uint32_t S,
                const int64_t* rec_end0, uint32_t n_rec0, const uint32_t* first, const uint64_t* piece_begin, uint32_t n_pieces,
                uint32_t* piece_row, int64_t* seg_len, int64_t* seg_start, uint8_t* keep, hipStream_t s) {
    if (!n_pieces) return;
    hipLaunchKernelGGL(k_cut_pieces, dim3(grid_for(n_pieces, 256)), dim3(256), 0, s, mom_len, mom_starts, mom_strands, m, S, rec_end0,
                       n_rec0, first, piece_begin, n_pieces, piece_row, seg_len, seg_start, keep);
    MMT_HIP(hipGetLastError());
}

// ---- locate and test --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t clamp_index(int64_t v, uint64_t n) {            // numpy's mode="clip"; n >= 1
    return v < 0 ? 0 : ((uint64_t)v >= n ? (int64_t)(n - 1) : v);
}

__global__ __launch_bounds__(256) void k_locate(const uint32_t* __restrict__ kept, uint32_t n_kept, uint32_t S,
                                                const int64_t* __restrict__ seg_len, const int64_t* __restrict__ seg_start,
                                                const PartView* __restrict__ parts, uint32_t* __restrict__ rec,
                                                int64_t* __restrict__ left_off, int64_t* __restrict__ right_off, uint8_t* __restrict__ ok) {
    const uint64_t total = (uint64_t)n_kept * S, stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const uint32_t q = (uint32_t)(t / S), i = (uint32_t)(t % S), p = kept[q];
        const PartView P = parts[i];
        const int64_t v = seg_start[(uint64_t)p * S + i], sl = seg_len[p];
        uint32_t rc = 0;
        int64_t lo = 0, ro = 0;
        bool good = false;
        if (P.n_rec && P.thresh_len) {
            const uint32_t r = upper_bound(P.rec_end, P.n_rec, v);
            rc = r < P.n_rec ? r : P.n_rec - 1;
            const int64_t begin = rc ? P.rec_end[rc - 1] : 0;
            lo = v - begin;
            ro = P.rec_end[rc] - v - sl - 1;
            const int64_t th = (int64_t)P.thresh[clamp_index(v, P.thresh_len)];
            good = r < P.n_rec && th != 0 && sl > th;
        }
        rec[t] = rc; left_off[t] = lo; right_off[t] = ro; ok[t] = good ? 1 : 0;
    }
}
void locate(const uint32_t* kept, uint32_t n_kept, uint32_t S, const int64_t* seg_len, const int64_t* seg_start, const PartView* parts,
            uint32_t* rec, int64_t* left_off, int64_t* right_off, uint8_t* ok, hipStream_t s) {
    if (!n_kept || !S) return;
    hipLaunchKernelGGL(k_locate, dim3(grid_capped((uint64_t)n_kept * S, 256)), dim3(256), 0, s, kept, n_kept, S, seg_len, seg_start,
                       parts, rec, left_off, right_off, ok);
    MMT_HIP(hipGetLastError());
}

__global__ __launch_bounds__(256) void k_all_ok(const uint8_t* __restrict__ ok, uint32_t n_kept, uint32_t S, uint8_t* __restrict__ all) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_kept) return;
    uint8_t a = 1;
    for (uint32_t i = 0; i < S; i++) a &= ok[(uint64_t)q * S + i];
    all[q] = a;
}
void all_ok(const uint8_t* ok, uint32_t n_kept, uint32_t S, uint8_t* all, hipStream_t s) {
    if (!n_kept) return;
    hipLaunchKernelGGL(k_all_ok, dim3(grid_for(n_kept, 256)), dim3(256), 0, s, ok, n_kept, S, all);
    MMT_HIP(hipGetLastError());
}

// ---- assemble ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_assemble(const uint32_t* __restrict__ kept, const uint32_t* __restrict__ sel, uint32_t n_sel,
                                                  uint32_t S, uint32_t C, const uint32_t* __restrict__ col_part,
                                                  const PartView* __restrict__ parts, const uint32_t* __restrict__ piece_row,
                                                  const uint8_t* __restrict__ mom_strands, const int64_t* __restrict__ seg_len,
                                                  const int64_t* __restrict__ seg_start, const uint32_t* __restrict__ rec,
                                                  const int64_t* __restrict__ left_off, const int64_t* __restrict__ right_off,
                                                  uint32_t* __restrict__ out_len, int64_t* __restrict__ out_starts,
                                                  uint8_t* __restrict__ out_strands, int64_t* __restrict__ base_fwd,
                                                  int64_t* __restrict__ base_rev, uint8_t* __restrict__ same, uint64_t* __restrict__ key,
                                                  uint32_t* __restrict__ val, unsigned long long* __restrict__ key_or) {
    const uint64_t total = (uint64_t)n_sel * C, stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long seen = 0;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const uint32_t row = (uint32_t)(t / C), col = (uint32_t)(t % C), i = col_part[col];
        const PartView P = parts[i];
        const uint32_t c = col - P.first_col, q = sel[row], p = kept[q];
        const uint64_t li = (uint64_t)q * S + i;
        const uint64_t cell = (uint64_t)rec[li] * P.n_cols + c;                  // (rec < n_rec <= n_rows, by the host)
        const bool fwd = P.strands[cell] != 0, matched_fwd = mom_strands[(uint64_t)piece_row[p] * S + i] != 0;
        const int64_t start = P.starts[cell] + (fwd ? left_off[li] : right_off[li]);
        out_starts[t] = start;
        out_strands[t] = matched_fwd == fwd ? 1 : 0;                              // the cell's strand, flipped for a reversed match
        if (c == 0) {
            const uint64_t lo = (uint64_t)row * S + i;
            const int64_t v = seg_start[(uint64_t)p * S + i];
            base_fwd[lo] = v;
            base_rev[lo] = v - left_off[li] + right_off[li];
            same[lo] = matched_fwd ? 1 : 0;
        }
        if (col == 0) {
            out_len[row] = (uint32_t)seg_len[p];
            key[row] = (uint64_t)start; val[row] = row;
            seen |= (unsigned long long)start;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)seen, o, 64), hi = __shfl_xor((uint32_t)(seen >> 32), o, 64);
        seen |= ((unsigned long long)hi << 32) | lo;
    }
    if ((threadIdx.x & 63) == 0 && seen) atomicOr(key_or, seen);
}
void assemble(const uint32_t* kept, const uint32_t* sel, uint32_t n_sel, uint32_t S, uint32_t C, const uint32_t* col_part,
              const PartView* parts, const uint32_t* piece_row, const uint8_t* mom_strands, const int64_t* seg_len,
              const int64_t* seg_start, const uint32_t* rec, const int64_t* left_off, const int64_t* right_off, uint32_t* out_len,
              int64_t* out_starts, uint8_t* out_strands, int64_t* base_fwd, int64_t* base_rev, uint8_t* same, uint64_t* key,
              uint32_t* val, uint64_t* key_or, hipStream_t s) {
    if (!n_sel || !C) return;
    hipLaunchKernelGGL(k_assemble, dim3(grid_capped((uint64_t)n_sel * C, 256)), dim3(256), 0, s, kept, sel, n_sel, S, C, col_part, parts,
                       piece_row, mom_strands, seg_len, seg_start, rec, left_off, right_off, out_len, out_starts, out_strands, base_fwd,
                       base_rev, same, key, val, reinterpret_cast<unsigned long long*>(key_or));
    MMT_HIP(hipGetLastError());
}

__global__ __launch_bounds__(256) void k_flip_sign(uint64_t* __restrict__ key, uint32_t n) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) key[r] ^= 1ull << 63;
}
void flip_sign(uint64_t* key, uint32_t n, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_flip_sign, dim3(grid_for(n, 256)), dim3(256), 0, s, key, n);
    MMT_HIP(hipGetLastError());
}

// ---- thresholds -------------------------------------------------------------------------------------------------------------
// LDS of a workgroup, for R rows at a time: R + 1 first output positions, R x S bases of either table, R lengths, R x S flags
constexpr uint8_t SAME = 1, SAFE = 2;          // the flags of a (row, partition) in LDS
__host__ __device__ inline uint32_t thresh_lds_bytes(uint32_t R, uint32_t S) { return (R + 1) * 8 + R * S * 16 + R * 4 + R * S; }
uint32_t thresholds_rows_at_once(uint32_t S) {
    uint32_t R = THRESH_MAX_ROWS;
    while (R && thresh_lds_bytes(R, S) > THRESH_LDS_BYTES) R >>= 1;
    return R;
}

__global__ __launch_bounds__(THRESH_BLOCK) void k_thresholds(const uint32_t* __restrict__ len, const uint64_t* __restrict__ row_begin,
                                                             const uint32_t* __restrict__ order, uint32_t n, uint32_t S, uint32_t R,
                                                             const int64_t* __restrict__ base_fwd, const int64_t* __restrict__ base_rev,
                                                             const uint8_t* __restrict__ same, const PartView* __restrict__ parts,
                                                             uint64_t n_out, uint16_t* __restrict__ out_fwd,
                                                             uint16_t* __restrict__ out_rev) {
    extern __shared__ __align__(16) unsigned char lds[];
    uint64_t* s_pos = reinterpret_cast<uint64_t*>(lds);                           // R + 1: where the row's positions begin in out
    int64_t* s_fwd = reinterpret_cast<int64_t*>(s_pos + R + 1);                   // R x S
    int64_t* s_rev = s_fwd + (size_t)R * S;                                       // R x S
    uint32_t* s_len = reinterpret_cast<uint32_t*>(s_rev + (size_t)R * S);         // R
    uint8_t* s_same = reinterpret_cast<uint8_t*>(s_len + R);                      // R x S
    // a workgroup takes a stretch of consecutive tiles: one search for the first, then every tile begins in the row the last ended in
    const uint64_t tiles = (n_out + THRESH_TILE - 1) / THRESH_TILE, share = (tiles + gridDim.x - 1) / gridDim.x;
    const uint64_t tile0 = blockIdx.x * share, tile1 = tile0 + share < tiles ? tile0 + share : tiles;
    if (tile0 >= tile1) return;                   // (uniform over the workgroup)
    // the last row that begins at or before the stretch's first position
    uint32_t lo = last_at_or_before(n, tile0 * THRESH_TILE, [&](uint32_t j) { return row_begin[j] + j; });
    for (uint64_t tile = tile0; tile < tile1; tile++) {
        const uint64_t p0 = tile * THRESH_TILE, p1 = p0 + THRESH_TILE < n_out ? p0 + THRESH_TILE : n_out;
        for (uint32_t jb = lo;;) {                // rows [jb, jb + cnt) and where the row behind them begins
            const uint32_t cnt = n - jb < R ? n - jb : R;
            __syncthreads();                      // (the rows of the round before are read until here)
            for (uint32_t k = threadIdx.x; k <= cnt; k += THRESH_BLOCK) s_pos[k] = row_begin[jb + k] + jb + k;   // row_begin[n] + n = n_out
            __syncthreads();
            uint32_t in = 1;                      // the rows of these that begin before the tile ends: the first one does
            while (in < cnt && s_pos[in] < p1) in++;
            for (uint32_t k = threadIdx.x; k < in; k += THRESH_BLOCK) s_len[k] = len[jb + k];
            // per (row, partition) the table behind the forward output and the one behind the reverse output (they change places
            // for a reversed match), each as the address of the row's first value when every position of the row lies inside the
            // table (SAFE: no clamping, one add per load), else as the index of that value (clamped position by position)
            for (uint32_t x = threadIdx.x; x < in * S; x += THRESH_BLOCK) {
                const uint32_t k = x / S, i = x % S;
                const uint64_t at = (uint64_t)order[jb + k] * S + i;
                const PartView P = parts[i];
                const int64_t bf = base_fwd[at], br = base_rev[at], L = (int64_t)len[jb + k];
                const bool sm = same[at] != 0;
                const bool safe = bf >= 0 && br >= 0 && (uint64_t)(bf + L) <= P.thresh_len && (uint64_t)(br + L) <= P.thresh_len;
                const int64_t fi = sm ? bf : br, ri = sm ? br : bf;
                const uint16_t* ft = sm ? P.thresh : P.thresh_rev;
                const uint16_t* rt = sm ? P.thresh_rev : P.thresh;
                s_fwd[x] = safe ? (int64_t)reinterpret_cast<uintptr_t>(ft + fi) : fi;
                s_rev[x] = safe ? (int64_t)reinterpret_cast<uintptr_t>(rt + ri) : ri;
                s_same[x] = (sm ? SAME : 0) | (safe ? SAFE : 0);
            }
            __syncthreads();
            const uint64_t from = s_pos[0] > p0 ? s_pos[0] : p0, to = s_pos[in] < p1 ? s_pos[in] : p1;
#pragma unroll 2
            for (uint32_t it = 0; it < THRESH_PER_ITEM; it++) {
                const uint64_t pos = p0 + it * THRESH_BLOCK + threadIdx.x;
                if (pos < from || pos >= to) continue;
                const uint32_t a = last_at_or_before(in, pos, [&](uint32_t k) { return s_pos[k]; });
                const uint32_t w = (uint32_t)(pos - s_pos[a]);     // (at most the row's length)
                uint32_t f_max = 0, r_max = 0;
                bool f_all = true, r_all = true;
                if (w == s_len[a]) {              // the 0 behind the row
                    f_all = r_all = false;
                } else {
                    for (uint32_t i = 0; i < S; i++) {
                        const uint32_t x = a * S + i;
                        uint32_t f, r;
                        if (s_same[x] & SAFE) {
                            f = reinterpret_cast<const uint16_t*>((uintptr_t)s_fwd[x])[w];
                            r = reinterpret_cast<const uint16_t*>((uintptr_t)s_rev[x])[w];
                        } else {
                            const PartView P = parts[i];
                            const bool sm = (s_same[x] & SAME) != 0;
                            f = (sm ? P.thresh : P.thresh_rev)[clamp_index(s_fwd[x] + (int64_t)w, P.thresh_len)];
                            r = (sm ? P.thresh_rev : P.thresh)[clamp_index(s_rev[x] + (int64_t)w, P.thresh_len)];
                        }
                        f_max = f > f_max ? f : f_max; r_max = r > r_max ? r : r_max;
                        f_all = f_all && f > 0; r_all = r_all && r > 0;
                    }
                }
                out_fwd[pos] = (uint16_t)(f_all ? f_max : 0);
                out_rev[pos] = (uint16_t)(r_all ? r_max : 0);
            }
            if (s_pos[in] >= p1) {                // the next tile begins in the last of these rows, or with the row behind them
                lo = s_pos[in] == p1 ? jb + in : jb + in - 1;
                break;
            }
            jb += in;                             // (in == cnt here, and jb + cnt < n: s_pos[cnt] < p1 <= n_out)
        }
    }
}
void thresholds(const uint32_t* len, const uint64_t* row_begin, const uint32_t* order, uint32_t n, uint32_t S, const int64_t* base_fwd,
                const int64_t* base_rev, const uint8_t* same, const PartView* parts, uint64_t n_out, uint16_t* out_fwd,
                uint16_t* out_rev, hipStream_t s) {
    if (!n || !n_out) return;
    const uint32_t R = thresholds_rows_at_once(S);   // (> 0: string_fold() refuses an S the LDS does not hold)
    hipLaunchKernelGGL(k_thresholds, dim3(grid_capped(n_out, THRESH_TILE, 4096)), dim3(THRESH_BLOCK), thresh_lds_bytes(R, S), s, len,
                       row_begin, order, n, S, R, base_fwd, base_rev, same, parts, n_out, out_fwd, out_rev);
    MMT_HIP(hipGetLastError());
}

}}  // namespace mmt::sk
