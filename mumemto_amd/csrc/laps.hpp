// laps.hpp -- HIP-event laps of the stages of a host routine (collinear.cpp, inversion.cpp); the events are read at the points
// where the host waits for the stream anyway.
#pragma once
#include <vector>

#include "device_utils.hpp"

namespace mmt {

class Laps {
public:
    Laps(hipStream_t s, float* ms) : s_(s), ms_(ms) {}
    ~Laps() { for (auto& l : open_) { (void)hipEventDestroy(l.a); (void)hipEventDestroy(l.b); } }
    void begin(int stage) {
        if (!ms_) return;
        Lap l; l.stage = stage;
        MMT_HIP(hipEventCreate(&l.a)); MMT_HIP(hipEventCreate(&l.b));
        MMT_HIP(hipEventRecord(l.a, s_));
        open_.push_back(l);
    }
    void end() { if (ms_) MMT_HIP(hipEventRecord(open_.back().b, s_)); }
    void collect() {                                  // after a stream synchronisation
        for (auto& l : open_) {
            float t = 0.f;
            MMT_HIP(hipEventElapsedTime(&t, l.a, l.b));
            ms_[l.stage] += t;
            (void)hipEventDestroy(l.a); (void)hipEventDestroy(l.b);
        }
        open_.clear();
    }
private:
    struct Lap { hipEvent_t a, b; int stage; };
    hipStream_t s_;
    float* ms_;
    std::vector<Lap> open_;
};

}  // namespace mmt
