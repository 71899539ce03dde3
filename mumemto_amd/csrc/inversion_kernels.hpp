// inversion_kernels.hpp -- device side of the inversion caller (mumemto/find_inversions.py find_reversals + inversion_coords
// on the block order of mumemto/utils.py:62 / :67).
//
// The reference orders the blocks of every column by the start of their first row (one argsort per column), looks for
// maximal stretches where the block number falls by one from position to position, keeps a stretch when every block of it
// lies on '-', and reads four coordinates off its first and last block.  Here a column whose block heads ascend is skipped
// (its order is the identity: no stretch), the others are sorted as (start, block) pairs, and one pass marks where stretches
// begin and end; stretches are disjoint and ordered, so the k-th begin belongs to the k-th end and nothing needs an atomic.
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

namespace mmt { namespace ik {

constexpr uint64_t STRAND_BIT = 1ull << 63;          // a key = start | strand << 63, as in collinear_kernels.hpp
constexpr uint32_t MARK_THREADS = 256;               // the mark pass: a workgroup takes MARK_THREADS x MARK_ITEMS positions
constexpr uint32_t MARK_ITEMS = 1;
constexpr uint32_t TABLE_PARTIAL = 1, TABLE_UNSORTED = 2, BLOCKS_BAD = 4;      // bits of *state below
constexpr uint32_t CALL_FIELDS = 5;                  // column, start, end, ref_start, ref_end

// *state |= TABLE_PARTIAL when a cell of the table is negative (-1 = absent), TABLE_UNSORTED when column 0 descends somewhere
void check_table(const int64_t* off, uint32_t n, uint32_t n_docs, uint32_t* state, hipStream_t s);
// *state |= BLOCKS_BAD unless every block has first <= last < n and begins behind the end of the block before it
void check_blocks(const uint32_t* lr, uint32_t n_blocks, uint32_t n, uint32_t* state, hipStream_t s);
// row_block[i] = the block whose rows include i, or 0xFFFFFFFF (the blocks are ascending and disjoint)
void rows_of_blocks(const uint32_t* lr, uint32_t n_blocks, uint32_t n, uint32_t* row_block, hipStream_t s);
// (the keys of the block heads come from ck::extract_block_heads, collinear_kernels.hpp)
// One column, n_blocks >= 2: order[j] = block at position j of the column, keys[j] its key.  dec[j] = order[j + 1] == order[j] - 1
// (j + 1 < n_blocks); head[j] = dec[j] and not dec[j - 1]; tail[j] = dec[j] and not dec[j + 1]; plus[j] = strand of order[j].
void mark(const uint32_t* order, const uint64_t* keys, uint32_t n_blocks, uint8_t* head, uint8_t* tail, uint32_t* plus,
          hipStream_t s);
// One thread per run k = positions heads[k] .. tails[k] + 1 of the column: plus_sum is the inclusive sum of plus.  rec[5 k ..]
// = (col, start, end, ref_start, ref_end) from the LAST row of the first block and the FIRST row of the last block;
// keep[k] = no '+' block in the run and (max_length < 0 or |end - start| <= max_length).
void emit(const uint32_t* heads, const uint32_t* tails, uint32_t n_runs, const uint32_t* order, const uint32_t* plus_sum,
          const uint32_t* lr, const int64_t* off, const uint32_t* length, uint32_t n_docs, uint32_t col, int64_t max_length,
          int64_t* rec, uint8_t* keep, hipStream_t s);
// out[5 k ..] = rec[5 sel[k] ..] for k < n_sel
void compact(const int64_t* rec, const uint32_t* sel, uint32_t n_sel, int64_t* out, hipStream_t s);

}}  // namespace mmt::ik
