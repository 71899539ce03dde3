// Our own stand-in for sdsl's bit-vector header, for the reference's include/ref_builder.hpp
// (oracle/_ref_drivers/mem_finder_driver.cpp).  RefBuilder holds a `bit_vector doc_ends` and a
// `rank_support_v<1> doc_ends_rank`; the scan only calls doc_ends_rank(i) = number of document
// ends at positions < i.  Here that rank is a binary search over the sorted end positions, so a
// document of billions of characters costs one entry.  No sdsl code is reproduced.
#ifndef MMT_SDSL_SHIM_BIT_VECTORS_HPP
#define MMT_SDSL_SHIM_BIT_VECTORS_HPP
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "io.hpp"

namespace sdsl {
struct bit_vector {};

template <uint8_t Bit = 1>
struct rank_support_v {
    std::vector<uint64_t> ends;          // sorted positions of the set bits
    size_t operator()(uint64_t i) const { return (size_t)(std::lower_bound(ends.begin(), ends.end(), i) - ends.begin()); }
    size_t rank(uint64_t i) const { return (*this)(i); }
};
}  // namespace sdsl
#endif
