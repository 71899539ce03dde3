// digest_kernels.hip -- see digest_kernels.hpp.  One streaming read of the message: 16-byte loads over the aligned body,
// scalar loads for the elements in front of and behind it, a wave reduction and one 64-bit atomic add + one atomic xor per
// workgroup and piece.  A workgroup is ONE wave, so the wave reduction is the workgroup's and nothing goes through LDS.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <stdexcept>

#include "device_utils.hpp"
#include "digest_kernels.hpp"

namespace mmt { namespace dk {

namespace {

constexpr unsigned long long GOLD = 0x9E3779B97F4A7C15ull, MUL1 = 0xBF58476D1CE4E5B9ull, MUL2 = 0x94D049BB133111EBull;
constexpr int WAVE = 64;
constexpr int UNROLL = 4;             // 16-byte loads a lane has in flight: 4 KiB per wave and step

// k = (i + 1) * GOLD
__device__ __forceinline__ unsigned long long mix(unsigned long long v, unsigned long long k) {
    unsigned long long x = v + k;
    x ^= x >> 30; x *= MUL1;
    x ^= x >> 27; x *= MUL2;
    x ^= x >> 31;
    return x;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int o = WAVE / 2; o; o >>= 1) v += __shfl_down(v, o, WAVE);
    return v;
}
__device__ __forceinline__ unsigned long long wave_xor(unsigned long long v) {
    for (int o = WAVE / 2; o; o >>= 1) v ^= __shfl_down(v, o, WAVE);
    return v;
}
// every lane of the wave calls this (p is the same in all of them)
__device__ __forceinline__ void flush(unsigned long long* __restrict__ out, unsigned long long p, unsigned long long s,
                                      unsigned long long x) {
    s = wave_sum(s); x = wave_xor(x);
    if (threadIdx.x == 0) { atomicAdd(out + 2 * p, s); atomicXor(out + 2 * p + 1, x); }
}

// element j of a 16-byte vector as T, zero-extended (j is a compile-time constant after unrolling)
template <typename T>
__device__ __forceinline__ unsigned long long element(const uint4& r, int j) {
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
    if (sizeof(T) == 1) return (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
    if (sizeof(T) == 4) return w[j];
    return (unsigned long long)w[2 * j] | ((unsigned long long)w[2 * j + 1] << 32);
}

// elements [lo, hi) of the message, one per lane (hi - lo <= 64): the scalar head and tail
template <typename T>
__device__ void digest_scalar(const T* __restrict__ buf, unsigned long long lo, unsigned long long hi, unsigned long long P,
                              unsigned long long* __restrict__ out) {
    if (lo >= hi) return;
    const unsigned long long e = lo + threadIdx.x;
    const bool have = e < hi;
    const unsigned long long v = have ? (unsigned long long)buf[e] : 0ull;
    for (unsigned long long p = lo / P, pl = (hi - 1) / P; p <= pl; p++) {
        const unsigned long long base = p * P;
        unsigned long long s = 0, x = 0;
        if (have && e >= base && e - base < P) { x = mix(v, (e - base + 1) * GOLD); s = x; }
        flush(out, p, s, x);
    }
}

template <typename T>
__global__ __launch_bounds__(WAVE) void k_digest_pieces(const T* __restrict__ buf, unsigned long long count, unsigned long long P,
                                                        unsigned long long head, unsigned long long nvec,
                                                        unsigned long long* __restrict__ out) {
    constexpr int VEC = 16 / sizeof(T);
    constexpr unsigned long long STEP = (unsigned long long)WAVE * UNROLL;       // vectors a wave takes per step
    const uint4* __restrict__ body = reinterpret_cast<const uint4*>(buf + head);
    const unsigned lane = threadIdx.x;
    // the piece this wave is inside of: its sums stay in registers until the wave leaves it
    bool open = false;
    unsigned long long cur = 0, cur_base = 0, cur_end = 0, s = 0, x = 0;
    const unsigned long long steps = (nvec + STEP - 1) / STEP;
    for (unsigned long long c = blockIdx.x; c < steps; c += gridDim.x) {
        const unsigned long long v0 = c * STEP, v1 = v0 + STEP < nvec ? v0 + STEP : nvec;
        const unsigned long long e0 = head + v0 * VEC, e1 = head + v1 * VEC;         // the step's elements: the same in every lane
        uint4 r[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            const unsigned long long vi = v0 + (unsigned long long)u * WAVE + lane;
            r[u] = vi < v1 ? body[vi] : make_uint4(0, 0, 0, 0);
        }
        bool inside = open && e0 >= cur_base && e1 <= cur_end;
        if (!inside) {
            if (open) { flush(out, cur, s, x); open = false; }
            const unsigned long long pf = e0 / P, pl = (e1 - 1) / P;
            if (pf == pl) {
                open = inside = true;
                cur = pf; cur_base = pf * P; cur_end = cur_base + P; s = 0; x = 0;
            } else {
                // a step that crosses piece boundaries (pieces of a few KiB: tests): piece by piece, each lane the elements of
                // its vectors that lie in it, read again one by one (rolled loops: this path must not cost the other registers)
                for (unsigned long long p = pf; p <= pl; p++) {
                    const unsigned long long base = p * P;
                    unsigned long long ps = 0, px = 0;
#pragma unroll 1
                    for (int u = 0; u < UNROLL; u++) {
                        const unsigned long long vi = v0 + (unsigned long long)u * WAVE + lane;
                        if (vi >= v1) continue;
#pragma unroll 1
                        for (int j = 0; j < VEC; j++) {
                            const unsigned long long e = head + vi * VEC + j;
                            if (e >= base && e - base < P) { const unsigned long long m = mix((unsigned long long)buf[e], (e - base + 1) * GOLD); ps += m; px ^= m; }
                        }
                    }
                    flush(out, p, ps, px);
                }
            }
        }
        if (inside) {
#pragma unroll
            for (int u = 0; u < UNROLL; u++) {
                const unsigned long long vi = v0 + (unsigned long long)u * WAVE + lane;
                if (vi >= v1) continue;
                unsigned long long k = (head + vi * VEC - cur_base + 1) * GOLD;
#pragma unroll
                for (int j = 0; j < VEC; j++) { const unsigned long long m = mix(element<T>(r[u], j), k); s += m; x ^= m; k += GOLD; }
            }
        }
    }
    if (open) flush(out, cur, s, x);
    if (blockIdx.x == 0) {
        digest_scalar<T>(buf, 0, head, P, out);
        digest_scalar<T>(buf, head + nvec * VEC, count, P, out);
    }
}

template <typename T>
void launch(const void* buf, uint64_t count, uint64_t P, uint64_t* out, hipStream_t st) {
    constexpr uint64_t VEC = 16 / sizeof(T);
    // elements in front of the first 16-byte boundary, whole vectors behind it; what is left is the tail (< VEC)
    const uint64_t to_boundary = ((16 - (reinterpret_cast<uintptr_t>(buf) & 15)) & 15) / sizeof(T);
    const uint64_t head = std::min<uint64_t>(to_boundary, count), nvec = (count - head) / VEC;
    const uint64_t steps = (nvec + (uint64_t)WAVE * UNROLL - 1) / ((uint64_t)WAVE * UNROLL);
    // 256 CUs x 16 waves, 4 KiB of loads each: 16 MiB in flight; the rest of the message by grid stride
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(steps, 4096));
    hipLaunchKernelGGL(k_digest_pieces<T>, dim3(grid), dim3(WAVE), 0, st, static_cast<const T*>(buf), (unsigned long long)count,
                       (unsigned long long)P, (unsigned long long)head, (unsigned long long)nvec,
                       reinterpret_cast<unsigned long long*>(out));
    MMT_HIP(hipGetLastError());
}

__global__ void k_compare_digests(const unsigned long long* __restrict__ a, const unsigned long long* __restrict__ b,
                                  unsigned long long n_pairs, unsigned long long pair_base, unsigned long long* __restrict__ res) {
    for (unsigned long long q = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; q < n_pairs;
         q += (unsigned long long)gridDim.x * blockDim.x) {
        if (a[2 * q] == b[2 * q] && a[2 * q + 1] == b[2 * q + 1]) continue;
        atomicAdd(res, 1ull);
        atomicMin(res + (q + 1 == n_pairs ? 2 : 1), pair_base + q);
    }
}

}  // namespace

void digest_pieces(const void* buf, uint64_t count, uint32_t width, uint64_t piece_elements, uint64_t* out, bool zero_out,
                   hipStream_t s) {
    if (width != 1 && width != 4 && width != 8) throw std::runtime_error("digest_pieces: width 1, 4 or 8");
    if (!piece_elements) throw std::runtime_error("digest_pieces: pieces of no elements");
    if (reinterpret_cast<uintptr_t>(buf) % width) throw std::runtime_error("digest_pieces: the buffer is not aligned to its elements");
    if (zero_out) MMT_HIP(hipMemsetAsync(out, 0, piece_count(count, piece_elements) * 16, s));
    if (!count) return;
    if (width == 1) launch<uint8_t>(buf, count, piece_elements, out, s);
    else if (width == 4) launch<uint32_t>(buf, count, piece_elements, out, s);
    else launch<uint64_t>(buf, count, piece_elements, out, s);
}

void compare_digests(const uint64_t* expected, const uint64_t* got, uint64_t n_pairs, uint64_t pair_base, uint64_t* res,
                     hipStream_t s) {
    if (!n_pairs) return;
    const unsigned grid = (unsigned)std::min<uint64_t>((n_pairs + 255) / 256, 1024);
    hipLaunchKernelGGL(k_compare_digests, dim3(grid), dim3(256), 0, s, reinterpret_cast<const unsigned long long*>(expected),
                       reinterpret_cast<const unsigned long long*>(got), (unsigned long long)n_pairs, (unsigned long long)pair_base,
                       reinterpret_cast<unsigned long long*>(res));
    MMT_HIP(hipGetLastError());
}

}}  // namespace mmt::dk
