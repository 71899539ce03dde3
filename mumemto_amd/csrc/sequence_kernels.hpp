// sequence_kernels.hpp -- device side of the multi-MUM sequence writer (the reference's src/extract_mums.cpp and
// mumemto/extract_mums.py: a substr / a Biopython slice per row, appended to one host string).
//
// Record k of a column is `>mum_<k>\n`, the bases of row k in that column, `#` unless told not to, and the separator.  The
// measure pass judges every row (what is refused, what is cut at the document's end, what is empty), gives the bytes of its
// record and keeps where its bases begin in the text; the format pass writes the records of a piece.  The text is read through
// TextRef (textref.hpp), so one kernel serves a byte per base and the packed layout, exception runs included.
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

#include "textref.hpp"

namespace mmt { namespace sq {

constexpr uint32_t CHUNK = 16;                  // bytes of one store: a lane owns aligned chunks of the piece buffer
constexpr uint32_t FORMAT_BLOCK = 256, FORMAT_ITEMS = 4;
constexpr uint32_t TILE_CHUNKS = FORMAT_BLOCK * FORMAT_ITEMS, TILE_BYTES = TILE_CHUNKS * CHUNK;      // 16 KB of text per tile
constexpr uint32_t LDS_RECORDS = 1024;          // record offsets of a tile a workgroup stages in LDS (8 KB); more: HBM is searched
constexpr uint64_t REVERSE = 1ull << 63;        // in source[k]: the record is the reverse complement of its range
constexpr uint64_t NO_ROW = ~0ull;

// flags (8 x u64, set up by clear_flags): the first row with a start below -1, the first row without a start (-1), the first
// row that starts beyond the document's end -- NO_ROW when there is none -- then the sums: bases written, rows cut at the
// document's end, empty records
enum Flag { BAD_START = 0, PARTIAL = 1, BEYOND = 2, BASES = 3, CLIPPED = 4, EMPTY = 5, N_FLAGS = 8 };
void clear_flags(uint64_t* flags, hipStream_t s);

struct Format {
    uint8_t upper = 0;          // bases are upper-cased (a-z only)
    uint8_t strands = 0;        // rows on '-' are reverse-complemented
    uint8_t terminator = 1;     // `#` behind the bases
    uint8_t join = 0;           // the separator stands between records, none behind the last one of the table
    uint8_t lenient = 0;        // a row without a start, or with one beyond the document's end, is an empty record, not a refusal
};

// Row k with start s = off[k * n_docs + col] in a document of doc_len bases whose first base is text position doc_begin:
// s < -1: BAD_START; s == -1 or s > doc_len: PARTIAL / BEYOND unless lenient, an empty record then; else min(length[k],
// doc_len - s) bases.  bytes[k] = 6 + digits(k) + bases + terminator + separator; source[k] = doc_begin + s, with REVERSE
// for a row on '-' when f.strands; bases[k] = the bases written.
void measure(const int64_t* off, const uint8_t* strands, const uint32_t* length, uint32_t n, uint32_t n_docs, uint32_t col,
             uint64_t doc_begin, uint64_t doc_len, Format f, uint64_t* bytes, uint64_t* source, uint32_t* bases, uint64_t* flags,
             hipStream_t s);

// The records [k0, k1) of a table of n at dst[0 ..): byte b of the text (offset[k] = where record k begins) goes to
// dst[b - base], base = offset[k0]; dst is 16-byte aligned.  The kernel reads the piece's bytes, offset[k1] - base, itself;
// bytes_at_most (the piece's bytes or more, the whole text's for one) sizes the launch alone.  The work is divided by output bytes: a lane assembles aligned
// chunks of 16 bytes in registers -- header, bases, terminator and newline of the one to three records the chunk falls into --
// and stores each with one 16-byte store; the bytes behind the last whole chunk are stored one by one by the lane that owns
// them.  A workgroup takes tiles of TILE_BYTES and finds the records of a tile once; its lanes search them in LDS (at most
// LDS_RECORDS) or in HBM.  The bases of a chunk are two aligned 16-byte reads of the text, shifted; a reverse record reads its
// range backwards and complements.
void format(const TextRef& T, const uint64_t* offset, const uint64_t* source, const uint32_t* bases, uint32_t k0, uint32_t k1,
            uint32_t n, uint64_t base, uint64_t bytes_at_most, Format f, char* dst, hipStream_t s);

}}  // namespace mmt::sq
