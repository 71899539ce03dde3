// base_pack.cpp -- see base_pack.hpp.
#include "base_pack.hpp"

#include "switches.hpp"

#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace mmt {
namespace {

// 0 1 2 3 for A C G T in either case, 4 for everything else
inline uint32_t code_of(uint8_t b) {
    switch (b) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': return 3;
        default: return 4;
    }
}

// the run list while it grows: exception bytes arrive in ascending positions; a run stays open while the same byte goes on
struct RunList {
    BaseRun* runs;
    size_t cap, n = 0;
    bool open = false, overflow = false;
    uint32_t start = 0, len = 0;
    uint8_t byte = 0;
    void close() {
        if (!open) return;
        open = false;
        if (n == cap) { overflow = true; return; }
        runs[n++] = BaseRun{start, len, byte};
    }
    void exception(uint32_t pos, uint8_t b) {
        if (open && byte == b && start + len == pos) { len++; return; }
        close();
        open = true; start = pos; len = 1; byte = b;
    }
};

// up to 32 bases from position pos on -> one word
inline uint64_t pack_word(const uint8_t* p, size_t count, uint32_t pos, RunList& R) {
    uint64_t w = 0;
    for (size_t k = 0; k < count; k++) {
        uint32_t c = code_of(p[k]);
        if (c > 3) { R.exception(pos + (uint32_t)k, p[k]); c = 0; }
        w |= (uint64_t)c << (2 * k);
    }
    return w;
}

size_t pack_tail(const uint8_t* in, size_t n, size_t from, uint64_t* words, RunList& R) {
    for (size_t i = from; i < n && !R.overflow; i += 32) words[i >> 5] = pack_word(in + i, n - i < 32 ? n - i : 32, (uint32_t)i, R);
    R.close();
    return R.overflow ? BASE_PACK_OVERFLOW : R.n;
}

}  // namespace

size_t pack_bases_scalar(const uint8_t* in, size_t n, uint64_t* words, BaseRun* runs, size_t run_cap) {
    if (n > 0xffffffffull) return BASE_PACK_OVERFLOW;
    RunList R{runs, run_cap};
    return pack_tail(in, n, 0, words, R);
}

#if defined(__x86_64__)
// 32 bases a time: one vector in, one word out.  A vector without exception bytes (all of them, nearly) costs a load, four
// compares, two multiply-adds and a shuffle; one with exceptions walks its mask, and a vector that continues the open run
// with 32 more of the same byte only lengthens it (a megabase of N is 32 K such vectors).
__attribute__((target("avx2")))
size_t pack_bases_avx2(const uint8_t* in, size_t n, uint64_t* words, BaseRun* runs, size_t run_cap) {
    if (n > 0xffffffffull) return BASE_PACK_OVERFLOW;
    RunList R{runs, run_cap};
    const __m256i fold = _mm256_set1_epi8((char)0xDF);           // (only a c g t reach A C G T by losing bit 5)
    const __m256i cA = _mm256_set1_epi8('A'), cC = _mm256_set1_epi8('C'), cG = _mm256_set1_epi8('G'), cT = _mm256_set1_epi8('T');
    const __m256i one = _mm256_set1_epi8(1), two = _mm256_set1_epi8(2), three = _mm256_set1_epi8(3);
    const __m256i pairs = _mm256_set1_epi16(0x0401), quads = _mm256_set1_epi32(0x00100001);
    const __m256i gather = _mm256_setr_epi8(0, 4, 8, 12, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
                                            0, 4, 8, 12, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1);
    size_t i = 0;
    for (; i + 32 <= n; i += 32) {
        const __m256i v = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(in + i));
        const __m256i u = _mm256_and_si256(v, fold);
        const __m256i isA = _mm256_cmpeq_epi8(u, cA), isC = _mm256_cmpeq_epi8(u, cC), isG = _mm256_cmpeq_epi8(u, cG),
                      isT = _mm256_cmpeq_epi8(u, cT);
        const __m256i code = _mm256_or_si256(_mm256_and_si256(isC, one), _mm256_or_si256(_mm256_and_si256(isG, two), _mm256_and_si256(isT, three)));
        const __m256i p16 = _mm256_maddubs_epi16(code, pairs);                // c0 + 4 c1: 4 bits per 16
        const __m256i p32 = _mm256_madd_epi16(p16, quads);                    // + 16 (c2 + 4 c3): one byte per 32
        const __m256i r = _mm256_shuffle_epi8(p32, gather);
        words[i >> 5] = (uint64_t)(uint32_t)_mm256_extract_epi32(r, 0) | ((uint64_t)(uint32_t)_mm256_extract_epi32(r, 4) << 32);
        const __m256i plain = _mm256_or_si256(_mm256_or_si256(isA, isC), _mm256_or_si256(isG, isT));
        uint32_t exc = ~(uint32_t)_mm256_movemask_epi8(plain);
        if (!exc) continue;
        if (exc == 0xffffffffu && R.open && R.start + R.len == (uint32_t)i &&
            (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(v, _mm256_set1_epi8((char)R.byte))) == 0xffffffffu) {
            R.len += 32;
            continue;
        }
        for (; exc; exc &= exc - 1) {
            const uint32_t k = (uint32_t)__builtin_ctz(exc);
            R.exception((uint32_t)i + k, in[i + k]);
        }
        if (R.overflow) return BASE_PACK_OVERFLOW;
    }
    return pack_tail(in, n, i, words, R);
}
bool pack_bases_cpu_has_avx2() { return __builtin_cpu_supports("avx2"); }
#else
size_t pack_bases_avx2(const uint8_t* in, size_t n, uint64_t* words, BaseRun* runs, size_t run_cap) {
    return pack_bases_scalar(in, n, words, runs, run_cap);
}
bool pack_bases_cpu_has_avx2() { return false; }
#endif

size_t pack_bases(const uint8_t* in, size_t n, uint64_t* words, BaseRun* runs, size_t run_cap) {
    static const bool avx2 = pack_bases_cpu_has_avx2() && !sw::on(sw::MUMEMTO_NO_AVX2);
    return avx2 ? pack_bases_avx2(in, n, words, runs, run_cap) : pack_bases_scalar(in, n, words, runs, run_cap);
}

}  // namespace mmt
