// string_fold_kernels.hpp -- device side of the string-based merge's last step (the reference's mumemto/merge_mums.py:211-307;
// the closed form it is held to is mumemto_amd/merge_mums.py string_merge).
//
// The MUMs of the partitions' extracted MUM strings ("MUMs of MUMs", mom) are cut where they span a `#` of collection 0, every
// piece is located in the record -- the MUM -- of every partition it lies in and tested against that partition's thresholds,
// the survivors become rows over all the partitions' columns in ascending order of column 0, and their thresholds are merged
// position by position.  Everything up to the table is proportional to the rows; k_thresholds is the pass over the positions.
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

namespace mmt { namespace sk {

constexpr uint32_t MIN_SEGMENT = 20;            // merge_mums.py:134,141: a shorter piece of a row cut at `#` is dropped
constexpr uint32_t THRESH_BLOCK = 256;          // work-items of a workgroup of the threshold pass
constexpr uint32_t THRESH_PER_ITEM = 8;         // output positions of a work-item, THRESH_BLOCK apart
constexpr uint32_t THRESH_TILE = THRESH_BLOCK * THRESH_PER_ITEM;   // consecutive output positions of a workgroup's tile
constexpr uint32_t THRESH_MAX_ROWS = 128;       // rows of a tile held in LDS at a time
constexpr uint32_t THRESH_LDS_BYTES = 48 * 1024;                   // what the rows held at a time may take

constexpr uint32_t PART_UNSORTED = 1, PART_ABSENT = 2;             // PartState.flags

// a partition in HBM; rec_end = the running sum of the lengths of its collection's records (one past every record's `#`)
struct PartView {
    const int64_t* starts;
    const uint8_t* strands;
    const uint16_t* thresh;
    const uint16_t* thresh_rev;
    const int64_t* rec_end;
    uint64_t thresh_len;
    uint32_t n_cols, first_col, n_rec;
};
struct PartState {
    uint32_t flags, pad;
    unsigned long long positions;               // the sum of length + 1 over the rows
};

// one pass over a table of n x n_cols starts: PART_ABSENT for a -1 anywhere, PART_UNSORTED where column 0 descends from one
// row to the next, the sum of len + 1 (len may be null: 0).  *state is zero before.
void check_table(const uint32_t* len, const int64_t* starts, uint32_t n, uint32_t n_cols, PartState* state, hipStream_t s);

// ---- split ----
// Row r of mom, begin s0 = starts[r * S] and length L: first[r] = the first `#` of collection 0 at or beyond s0, pieces[r] = 1 +
// the `#`s in [s0, s0 + L); `#` k lies at rec_end0[k] - 1.
void count_pieces(const uint32_t* mom_len, const int64_t* mom_starts, uint32_t m, uint32_t S, const int64_t* rec_end0, uint32_t n_rec0,
                  uint32_t* first, uint32_t* pieces, hipStream_t s);
// Piece p, the k-th of row r (piece_begin: the exclusive sum of pieces, m + 1 entries): left = 0 or one past the `#` before it,
// end = L or the `#` behind it, both relative to s0; seg_len[p] = end - left, keep[p] = seg_len >= MIN_SEGMENT or the row has
// one piece; seg_start[p * S + i] = starts[r * S + i] + left where the row matched forward in collection i, + (L - end) where
// reversed; piece_row[p] = r.
void cut_pieces(const uint32_t* mom_len, const int64_t* mom_starts, const uint8_t* mom_strands, uint32_t m, uint32_t S,
                const int64_t* rec_end0, uint32_t n_rec0, const uint32_t* first, const uint64_t* piece_begin, uint32_t n_pieces,
                uint32_t* piece_row, int64_t* seg_len, int64_t* seg_start, uint8_t* keep, hipStream_t s);

// ---- locate and test ----
// Kept piece q = kept[q] of the pieces, partition i, v = seg_start: rec[q * S + i] = the record v lies in (the first whose end
// is beyond v, the last one when there is none), left_off = v - the record's begin, right_off = the record's end - v - seg_len
// - 1, ok = the record exists and 0 != thresh_i[clamp(v)] < seg_len.
void locate(const uint32_t* kept, uint32_t n_kept, uint32_t S, const int64_t* seg_len, const int64_t* seg_start, const PartView* parts,
            uint32_t* rec, int64_t* left_off, int64_t* right_off, uint8_t* ok, hipStream_t s);
// all[q] = the AND of ok[q * S ..][0 .. S)
void all_ok(const uint8_t* ok, uint32_t n_kept, uint32_t S, uint8_t* all, hipStream_t s);

// ---- assemble ----
// Surviving piece t = kept[sel[t]], C = the columns of all partitions, col_part[col] = the partition of a column: cell (t, col)
// is the start of the located row of that partition in that column + left_off on a `+` cell, + right_off on a `-` cell; the
// strand is the cell's, flipped where the piece matched reversed in the partition's collection.  Row-major, consecutive
// work-items write consecutive cells.  Per (t, partition): base_fwd = seg_start, base_rev = the record's begin + right_off
// (where the piece's thresholds begin in thresh_i and thresh_rev_i), same = the piece matched forward.  key[t] = column 0,
// val[t] = t, *key_or |= every key.
void assemble(const uint32_t* kept, const uint32_t* sel, uint32_t n_sel, uint32_t S, uint32_t C, const uint32_t* col_part,
              const PartView* parts, const uint32_t* piece_row, const uint8_t* mom_strands, const int64_t* seg_len,
              const int64_t* seg_start, const uint32_t* rec, const int64_t* left_off, const int64_t* right_off, uint32_t* out_len,
              int64_t* out_starts, uint8_t* out_strands, int64_t* base_fwd, int64_t* base_rev, uint8_t* same, uint64_t* key,
              uint32_t* val, uint64_t* key_or, hipStream_t s);
// keys of signed starts for an unsigned sort: the sign bit flipped
void flip_sign(uint64_t* key, uint32_t n, hipStream_t s);

// ---- thresholds ----
// Rows [0, n) in their final order, row_begin = the exclusive sum of len (n + 1 entries): row j owns the output positions
// row_begin[j] + j + [0, len[j]] -- its positions and one terminating 0.  For position w of row j, t = order[j], over the
// partitions i: a = thresh_i[clamp(base_fwd[t * S + i] + w)], b = thresh_rev_i[clamp(base_rev[t * S + i] + w)], swapped where
// same[t * S + i] is 0; out_fwd = the maximum of the a when every a > 0, else 0, out_rev the same of the b.  A workgroup takes
// a stretch of consecutive tiles of THRESH_TILE output positions: the first row of the first tile by one search, then the rows
// from there, from tile to tile, thresholds_rows_at_once(S) at a time in LDS: per row and partition the two tables behind the
// forward and the reverse output, as the addresses of the row's first values where no position of the row needs clamping (else
// as indices, clamped position by position), and a flag byte.  A work-item finds the row of each of its THRESH_PER_ITEM
// positions among those, reads 2 * S values at addresses consecutive with its neighbours' and writes two.  No atomics.
uint32_t thresholds_rows_at_once(uint32_t S);            // 0: S is too large for the LDS (the caller refuses before it calls)
void thresholds(const uint32_t* len, const uint64_t* row_begin, const uint32_t* order, uint32_t n, uint32_t S, const int64_t* base_fwd,
                const int64_t* base_rev, const uint8_t* same, const PartView* parts, uint64_t n_out, uint16_t* out_fwd,
                uint16_t* out_rev, hipStream_t s);

}}  // namespace mmt::sk
