// base_pack.hpp -- the bases of a FASTA chunk at two bits each, for the trip over the host link.
//
// What reaches the text is A, C, G, T plus rare runs of something else (every reader of the document slots upper-cases:
// kernels.hip k_build_text), so a chunk of bases crosses the link as
//   * words: base k of the chunk in bits [2 (k & 31), + 2) of word k >> 5, codes A C G T -> 0 1 2 3 as in textref.hpp
//     (code order = byte order); a c g t fold to the same codes; the bits behind the last base are zero;
//   * runs: every other byte value packs as code 0 and is listed -- maximal runs of ONE byte value, kept verbatim ('n' stays
//     'n': the text builder upper-cases it as it always did), as (start within the chunk, length, byte), ascending.
// k::unpack_bases (kernels.hpp) writes the bytes back on the device.  No HIP in here: host tools and stand-alone test
// programs include it (tests/base_pack_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

namespace mmt {

struct BaseRun { uint32_t start, len, byte; };            // chunk positions [start, start + len) hold `byte`

// the most runs a caller may ask for per chunk (what its staging buffers are sized for): a chunk with more goes raw
constexpr size_t BASE_PACK_RUN_CAP = 16384;
constexpr size_t BASE_PACK_OVERFLOW = ~(size_t)0;

inline size_t base_pack_words(size_t n) { return (n + 31) / 32; }

// in[0 .. n) -> words[0 .. base_pack_words(n)) and runs[0 .. returned); BASE_PACK_OVERFLOW when the chunk holds more than
// run_cap runs (nothing is written beyond runs[run_cap - 1]) or n does not fit 32 bits.  `in` has any alignment.
size_t pack_bases(const uint8_t* in, size_t n, uint64_t* words, BaseRun* runs, size_t run_cap);

// the two bodies behind it, the same output bit for bit: pack_bases takes the AVX2 one where the CPU has it and
// MUMEMTO_NO_AVX2 is not set (as fasta.cpp chooses its line copier)
size_t pack_bases_scalar(const uint8_t* in, size_t n, uint64_t* words, BaseRun* runs, size_t run_cap);
size_t pack_bases_avx2(const uint8_t* in, size_t n, uint64_t* words, BaseRun* runs, size_t run_cap);   // (scalar where there is no AVX2 to compile for)
bool pack_bases_cpu_has_avx2();

}  // namespace mmt
