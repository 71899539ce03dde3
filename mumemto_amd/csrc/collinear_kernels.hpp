// collinear_kernels.hpp -- device side of the collinear blocks of multi-MUMs (mumemto/utils.py:9-64 find_coll_blocks).
//
// The reference ranks every row in every column (one argsort per column) and compares rank differences of consecutive rows.
// Here no rank exists: in the sorted order of column j two NEIGHBOURS a, b certify the pair of rows (min(a, b), min(a, b) + 1)
// in that column when they are consecutive rows in the direction their common strand asks for.  Every pair has at most one
// writer per column, so a per-pair count of agreeing columns and a per-pair running maximum of the gaps need no atomics
// while the columns run in stream order.
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

namespace mmt { namespace ck {

constexpr uint32_t NO_BLOCK = 0xffffffffu;
constexpr uint64_t STRAND_BIT = 1ull << 63;          // a column key = start | strand << 63
constexpr int64_t NO_GAP = INT64_MIN;

// flags[r] = row r has no -1 in any column; one wave per row
void full_row_flags(const int64_t* off, uint32_t n, uint32_t n_docs, uint8_t* flags, hipStream_t s);
// keys[k] = offsets[rows[k] * n_docs] (column 0 of the kept rows); *unsorted |= 1 when they are not non-decreasing
void anchor_keys(const int64_t* off, const uint32_t* rows, uint32_t m, uint32_t n_docs, uint64_t* keys, uint32_t* unsorted,
                 hipStream_t s);
// Columns [c0, c0 + n_cols) of the row-major table as n_cols arrays of n keys (start | strand << 63), through a tile
// transpose in LDS: rows are read n_cols x 8 contiguous bytes at a time, columns are written 64 keys at a time.
// col_state[c - c0] |= 1 when column c is not non-decreasing; *key_or |= every start (its width is the sort's bit range;
// bit 63 set = a negative start).  col_state and key_or must be zero on entry.
void extract_columns(const int64_t* off, const uint8_t* st, uint32_t n, uint32_t n_docs, uint32_t c0, uint32_t n_cols,
                     uint64_t* keys, uint32_t* col_state, uint64_t* key_or, hipStream_t s);
// the same over the FIRST rows lr[2 b] of the n_blocks blocks: n_cols arrays of n_blocks keys (the inversion caller's block heads)
void extract_block_heads(const int64_t* off, const uint8_t* st, const uint32_t* lr, uint32_t n_blocks, uint32_t n_docs, uint32_t c0,
                         uint32_t n_cols, uint64_t* keys, uint32_t* col_state, uint64_t* key_or, hipStream_t s);
void iota(uint32_t* v, uint32_t n, hipStream_t s);
// One column: keys in ascending order of the start, perm[k] = row of keys[k] (null: the column was ascending already, the
// identity).  Neighbours a = perm[k], b = perm[k + 1]: b == a + 1 and both '+' certify pair a, b == a - 1 and both '-' certify
// pair b; the gap of the column is start[k + 1] - start[k] - length[a] (the lower start is always a's).
void adjacency(const uint64_t* keys, const uint32_t* perm, const uint32_t* length, uint32_t n, uint32_t* pair_cols,
               int64_t* pair_gap, hipStream_t s);
void pair_init(uint32_t* pair_cols, int64_t* pair_gap, uint32_t n, hipStream_t s);
// starts[i] = 1 where a block begins at row i (a run of good pairs, or a singleton: a row in no run with length >= min_single,
// min_single < 0: none); a pair is good when every column agreed and, with max_break > 0, no gap exceeds it
void block_starts(const uint32_t* pair_cols, const int64_t* pair_gap, const uint32_t* length, uint32_t n, uint32_t n_docs,
                  uint32_t max_break, int64_t min_single, uint32_t* starts, hipStream_t s);
// numbered[i] = inclusive sum of starts: row_block[i] = block of row i or NO_BLOCK, lr[2 b] / lr[2 b + 1] = first / last row of b
void block_rows(const uint32_t* pair_cols, const int64_t* pair_gap, const uint32_t* length, const uint32_t* numbered, uint32_t n,
                uint32_t n_docs, uint32_t max_break, int64_t min_single, uint32_t* row_block, uint32_t* lr, hipStream_t s);

}}  // namespace mmt::ck
