// launch_grid.hpp -- the number of workgroups of a launch, for every launch wrapper.
#pragma once
#include <cstdint>
#include <string>

#include "device_utils.hpp"

namespace mmt {

// A launch may not have 2^32 work-items or more (HIP folds the product of grid and workgroup size into 32 bits: a
// larger launch silently runs a fraction of its workgroups).  Every kernel here uses workgroups of at most 256
// work-items with grid_for, so 2^24 workgroups is the limit; kernels over text-sized ranges handle 4 - 16 items per
// work-item and stay below it for any text that fits the device.
inline unsigned grid_for(uint64_t items, unsigned per_block) {
    uint64_t g = (items + per_block - 1) / per_block;
    if (g >= (1ull << 24)) throw HipError("kernel launch of 2^32 work-items or more (" + std::to_string(items) + " items)");
    return (unsigned)(g ? g : 1);
}
// for grid-stride kernels: a launch stays far below 2^32 work-items for any count below 2^32
inline unsigned grid_capped(uint64_t items, unsigned per_block, uint64_t cap = 1ull << 20) {
    const uint64_t g = (items + per_block - 1) / per_block;
    return (unsigned)(g ? (g < cap ? g : cap) : 1);
}

}  // namespace mmt
