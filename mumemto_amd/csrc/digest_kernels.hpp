// digest_kernels.hpp -- per-piece digests of a message of the multi-GPU exchange (dist.cpp).
//
// A message of `count` elements (1, 4 or 8 bytes wide) travels as pieces of `piece_elements` elements, cut as send_pieces /
// recv_pieces cut it (a message of no elements is still one piece).  The digest of a piece is two 64-bit words: with v the
// value of element i of the piece (0-based INSIDE the piece), zero-extended to 64 bits, everything mod 2^64:
//     x = v + (i + 1) * 0x9E3779B97F4A7C15;  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;
//     x ^= x >> 31;  sum += x;  xor ^= x
// Position-dependent (swapped halves and shifted data change it), commutative (any grid gives the same words) and a function
// of values and in-piece indices only -- never of the buffer's address or alignment.
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

namespace mmt { namespace dk {

inline uint64_t piece_count(uint64_t count, uint64_t piece_elements) {
    return count ? (count + piece_elements - 1) / piece_elements : 1;
}

// out[2 p] = sum word, out[2 p + 1] = xor word of piece p, p < piece_count(count, piece_elements): device memory, ONE launch
// per message.  zero_out: clear the words first (stream-ordered); a caller that digests many messages into one array clears
// it once itself.  width 1, 4 or 8; buf aligned to its element width; piece_elements >= 1.
void digest_pieces(const void* buf, uint64_t count, uint32_t width, uint64_t piece_elements, uint64_t* out, bool zero_out,
                   hipStream_t s);

// pairs of digest words against each other: res[0] += pairs that differ, res[1] = min(res[1], pair_base + q) over the
// differing DATA pairs q < n_pairs - 1, res[2] = min(res[2], pair_base + n_pairs - 1) if the LAST pair (the digest of the
// trailer itself) differs.
void compare_digests(const uint64_t* expected, const uint64_t* got, uint64_t n_pairs, uint64_t pair_base, uint64_t* res,
                     hipStream_t s);

}}  // namespace mmt::dk
