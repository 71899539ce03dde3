// coverage_kernels.hpp -- device side of the multi-MUM coverage of a sequence (mumemto/mum_coverage.py: one bool per base,
// a slice set per row, the set bits counted).
//
// Here no bitmap exists: the cells of a column are half-open intervals [start, min(start + length, L)), and in ascending
// order of the start, with prev = the maximum of all earlier ends, an interval adds max(0, end - max(start, prev)) covered
// positions and begins a new run of covered positions when start > prev.  Both arrays are kept shifted by one, b = start + 1
// and e = end + 1, so that 0 means "none": e = 0 is the identity of the running maximum, adds nothing and begins nothing, and
// the first interval of a column (prev = 0) always begins a run.  An absent cell is (0, 0) and sorts to the front; a cell that
// the length filter or the end of the sequence drops is (b, 0): it keeps its begin, so that a column whose starts ascend still
// ascends and needs no sort.
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

namespace mmt { namespace cvk {

constexpr uint32_t SCAN_BLOCK = 256, SCAN_ITEMS = 8, SCAN_TILE = SCAN_BLOCK * SCAN_ITEMS;   // elements of one workgroup
inline uint32_t scan_tiles(uint32_t n) { return (uint32_t)(((uint64_t)n + SCAN_TILE - 1) / SCAN_TILE); }

// Columns [c0, c0 + n_cols) of the row-major table as n_cols arrays of n begins and n ends, through a tile transpose in LDS:
// rows are read n_cols x 8 contiguous bytes at a time, columns are written 64 entries at a time.  A cell is absent, (0, 0),
// when its start is -1, and dropped, (b, 0), when length[row] < min_length or when it starts at or beyond seq_len[column]; an
// end beyond seq_len[column] is clipped to it.  col_state[c - c0] |= 1 when the begins of column c are not non-decreasing;
// *key_or |= every begin and every start other than -1 (its width is the sort's bit range; bit 62 or 63 set = a start out
// of range).  col_state and key_or must be zero on entry.
void extract_intervals(const int64_t* off, const uint32_t* length, const int64_t* seq_len, uint32_t n, uint32_t n_docs,
                       uint32_t c0, uint32_t n_cols, int64_t min_length, uint64_t* begins, uint64_t* ends,
                       uint32_t* col_state, uint64_t* key_or, hipStream_t s);

// The running maximum of the ends of one column, in three launches; no workgroup waits for another.
// (1) tile_max[t] = maximum of the ends of tile t
void tile_max(const uint64_t* ends, uint32_t n, uint64_t* tile_max, hipStream_t s);
// (2) one workgroup: carry[t] = maximum of tile_max[0 .. t) (0 for t = 0)
void tile_carry(const uint64_t* tile_max, uint32_t tiles, uint64_t* carry, hipStream_t s);
// (3) per element, with prev = the maximum of all ends before it: ends[i] = prev (in place), heads[i] = it is an interval and
// begins[i] > prev, *covered += max(0, end - max(begin, prev)) (one 64-bit integer atomic per workgroup: exact in any
// order), *n_heads += the heads, *col_max = the maximum of all ends (written by the workgroup of the last element)
void apply_prev(const uint64_t* begins, uint64_t* ends, const uint64_t* carry, uint32_t n, uint32_t* heads, uint64_t* covered,
                uint32_t* n_heads, uint64_t* col_max, hipStream_t s);
// numbered[i] = exclusive sum of heads.  A head writes its begin as runs[2 r], r = numbered[i], and for r > 0 its prev as the
// end of run r - 1, runs[2 (r - 1) + 1]; the last element writes *col_max as the end of the last run.  (Values unshifted.)
void write_runs(const uint64_t* begins, const uint64_t* prevs, const uint32_t* heads, const uint32_t* numbered, uint32_t n,
                const uint64_t* col_max, int64_t* runs, hipStream_t s);

}}  // namespace mmt::cvk
