// density_check.cpp -- the slice rule of csrc/density_kernels.hpp on the host (tests/test_density_host.py): reads lines of
// `start l size` and prints `a b cut` for each.  Built with the host sanitizers; the kernels call the same function.
#include <cinttypes>
#include <cstdio>

#include "density_kernels.hpp"

int main() {
    long long start, l, size;
    while (std::scanf("%lld %lld %lld", &start, &l, &size) == 3) {
        const mmt::dnk::Slice s = mmt::dnk::slice_of((int64_t)start, (uint32_t)l, (int64_t)size);
        std::printf("%" PRId64 " %" PRId64 " %d\n", s.a, s.b, s.cut ? 1 : 0);
    }
    return 0;
}
