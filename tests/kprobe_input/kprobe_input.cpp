// kprobe_input.cpp -- test infrastructure: a plain C entry point around k::unpack_bases (kernels.hpp), the device half of
// the two-bit transport of FASTA chunks (base_pack.hpp), for tests/test_gpu_packed_input.py.  In the manner of
// tests/kprobe/kprobe.cpp: host arrays go up, exactly ONE wrapper is called, the results come back; the in/out array goes up
// as the caller filled it, so what the wrapper must not touch comes back unchanged.  Errors: a non-zero return code, the
// message through kpi_last_error().  The library links the product's own objects; nothing of the product is restated here.
#include <cstdint>
#include <stdexcept>
#include <string>

#include <hip/hip_runtime.h>

#include "device_utils.hpp"
#include "kernels.hpp"

using namespace mmt;

#define KP extern "C" __attribute__((visibility("default")))

static std::string g_err;

// device memory for the length of one call
struct Mem {
    void* p = nullptr;
    explicit Mem(size_t bytes) { MMT_HIP(hipMalloc(&p, bytes ? bytes : 1)); }
    ~Mem() { (void)hipFree(p); }
    Mem(const Mem&) = delete;
};
static void need(bool ok, const char* what) { if (!ok) throw std::runtime_error(std::string("kprobe precondition: ") + what); }

KP const char* kpi_last_error() { return g_err.c_str(); }

// buf: in/out, buf_len bytes; the wrapper writes buf[at .. at + n) on the device, whose copy of buf starts at a 16-byte
// boundary (so at % 16 is the destination's misalignment); runs: n_runs triples (start, length, byte) as base_pack.hpp has them
KP int kpi_unpack_bases(const uint64_t* words, uint32_t n_words, uint32_t n, const uint32_t* runs, uint32_t n_runs, uint8_t* buf,
                        uint32_t buf_len, uint32_t at) {
    try {
        need(n_words >= (n + 31) / 32, "words cover n bases");
        need((uint64_t)at + n <= buf_len, "the destination lies inside buf");
        static_assert(sizeof(BaseRun) == 3 * sizeof(uint32_t), "a run is three 32-bit values");
        Mem w((size_t)n_words * 8), r((size_t)n_runs * 12), b(buf_len);
        need((reinterpret_cast<uintptr_t>(b.p) & 15) == 0, "device buffers start at a 16-byte boundary");
        if (n_words) MMT_HIP(hipMemcpy(w.p, words, (size_t)n_words * 8, hipMemcpyHostToDevice));
        if (n_runs) MMT_HIP(hipMemcpy(r.p, runs, (size_t)n_runs * 12, hipMemcpyHostToDevice));
        if (buf_len) MMT_HIP(hipMemcpy(b.p, buf, buf_len, hipMemcpyHostToDevice));
        k::unpack_bases(static_cast<const uint64_t*>(w.p), n, static_cast<const BaseRun*>(r.p), n_runs, static_cast<uint8_t*>(b.p) + at, nullptr);
        MMT_HIP(hipDeviceSynchronize());
        if (buf_len) MMT_HIP(hipMemcpy(buf, b.p, buf_len, hipMemcpyDeviceToHost));
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
    catch (...) { g_err = "unknown error"; return 2; }
}
