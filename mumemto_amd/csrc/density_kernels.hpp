// density_kernels.hpp -- device side of the MEM density of the sequences (mumemto/mem_density.py: a num x size array of
// float64, `coverage[idx, start:start+l] += 1` per occurrence).
//
// Here no per-base array has to exist.  The sequences are cut into bins of W positions, bin k = [kW, hi(k)) with
// hi(k) = min((k + 1) W, size), and an occurrence posts two events into two tables of num x nbins 64-bit integers, C and E:
// where its interval [a, b) begins, C[bin(a)] += 1 and E[bin(a)] += hi(bin(a)) - a; where it ends, C[bin(b)] -= 1 and
// E[bin(b)] -= hi(bin(b)) - b.  With P the exclusive sum of C along a sequence, the depth summed over bin k is
// E[k] + (hi(k) - kW) * P[k]: P counts the intervals that began in an earlier bin and have not ended before this one, each
// of which covers the bin whole, and E corrects the two bins an interval begins and ends in.  For W = 1 this is the plain
// difference array.  An interval that ends at `size` posts no end event: nothing lies behind it (its bin would be nbins
// when W divides size).  All sums are integer atomics, exact in any order.
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

// 1: a workgroup's events go through a table in LDS before they reach the tables in HBM; 0: every event is two atomics on
// HBM (the yardstick of tests/density_timing.py; DESIGN.md 9a has the figures, and why lanes of a wave are not combined first).
#ifndef DENSITY_PREAGG
#define DENSITY_PREAGG 1
#endif

namespace mmt { namespace dnk {

// The slice rule of numpy on an axis of `size` entries for start : start + l (l >= 0): a negative index counts from the end,
// and both ends are clamped into [0, size].  Empty when a >= b.
struct Slice { int64_t a, b; bool cut; };
#if defined(__HIPCC__)
__host__ __device__
#endif
inline Slice slice_of(int64_t start, uint32_t l, int64_t size) {
    Slice s;
    s.cut = false;
    if (start >= 0) {
        if (start >= size) { s.a = s.b = size; s.cut = start > size || l > 0; return s; }
        s.a = start;
        s.cut = (int64_t)l > size - start;
        s.b = s.cut ? size : start + (int64_t)l;
        return s;
    }
    s.a = start + size > 0 ? start + size : 0;
    const int64_t stop = start + (int64_t)l;                   // (no overflow: start < 0)
    if (stop < 0) s.b = stop + size > 0 ? stop + size : 0;
    else { s.cut = stop > size; s.b = s.cut ? size : stop; }
    return s;
}

// counters of the add pass, summed over every call: occurrences, occurrences whose stop lay beyond `size` (cut there),
// occurrences that covered nothing, occurrences with a negative start
constexpr int N_COUNTERS = 4;

// One lane per occurrence i of the flat list, n_occ of them; the row of i is the last r with occ_start[r] <= i (occ_start:
// n_rows < 2^32 entries, ascending, occ_start[0] = 0; rows without occurrences are legal).  A workgroup finds the rows of the first
// and the last occurrence of its tile once, each lane then searches between the two.  docs[i] < num for every i.
// C and E: num x nbins entries each, nbins = ceil(size / W).
void add(const uint32_t* length, const uint64_t* occ_start, uint64_t n_rows, const int64_t* starts, const uint64_t* docs,
         uint64_t n_occ, int64_t size, uint64_t W, uint64_t nbins, uint64_t* C, uint64_t* E, uint64_t* counters,
         hipStream_t s);

// base[q] = sums[q * nbins] for the num sequences: the running sum of C over the flat table at the head of each sequence
void row_base(const uint64_t* sums, uint64_t num, uint64_t nbins, uint64_t* base, hipStream_t s);
// in place over the flat table: out[i] = E[i] + (hi(k) - kW) * (out[i] - base[q]), q = i / nbins, k = i % nbins
void finish(const uint64_t* E, const uint64_t* base, uint64_t num, uint64_t nbins, int64_t size, uint64_t W, uint64_t* out,
            hipStream_t s);

}}  // namespace mmt::dnk
