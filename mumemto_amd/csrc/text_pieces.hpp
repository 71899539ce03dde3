// text_pieces.hpp -- a text of whole lines that leaves the device in pieces: what write_merged_text (merge.cpp),
// label_write_text and bed_write_text share.  A measure kernel gives the bytes of every line; line_offsets places them;
// write_text_pieces cuts them into pieces of whole lines (piece_cut.hpp), has the caller format every piece into one of two
// device buffers and hands it to a PieceWriter, which writes it to the file while the next one is formatted.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>

#include "device_utils.hpp"
#include "laps.hpp"
#include "piece_cut.hpp"

namespace mmt {

// bytes: n per-line byte counts and room for one more entry; offset: n + 1 entries.  Zeroes bytes[n], offset = the exclusive
// sum of the n + 1 counts (offset[n] = all bytes), and returns that total (waits for the stream).
uint64_t line_offsets(DevBuf<uint8_t>& temp, uint32_t* bytes, uint64_t* offset, size_t n, hipStream_t st);
uint64_t line_offsets(DevBuf<uint8_t>& temp, uint64_t* bytes, uint64_t* offset, size_t n, hipStream_t st);

// the piece size of a text writer: dflt, or what the test hook MMT_MERGED_TEXT_PIECE says (at least 4096)
size_t text_piece_bytes(size_t dflt);

// launches the caller's write kernel: the lines [k0, k1), whose first byte is byte `base` of the text, at dst[0 ..)
using PieceFormat = std::function<void(size_t k0, size_t k1, uint64_t base, char* dst)>;

// event laps around the format and around the copy of every piece (a stage < 0: none); collected before the file closes
struct PieceLaps { Laps* laps = nullptr; int format = -1, copy = -1; };

// Writes the n lines at d_offset (n + 1 device offsets, d_offset[n] = bytes) to path, in pieces of at most piece_bytes.  A
// text that fits one piece does not bring its offsets to the host.  Returns the milliseconds the host waited for the file:
// for room in the ring, and for the close.
double write_text_pieces(hipStream_t st, int device, const uint64_t* d_offset, size_t n, uint64_t bytes, size_t piece_bytes,
                         const std::string& path, const PieceFormat& format, PieceLaps laps = PieceLaps());

}  // namespace mmt
