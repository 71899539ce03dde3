// text_pieces.cpp -- see text_pieces.hpp.
#include "text_pieces.hpp"

#include <algorithm>
#include <chrono>
#include <vector>

#include "piece_writer.hpp"
#include "prims.hpp"
#include "switches.hpp"

namespace mmt {
namespace {

uint64_t read_total(const uint64_t* at, hipStream_t st) {
    uint64_t total = 0;
    MMT_HIP(hipMemcpyAsync(&total, at, 8, hipMemcpyDeviceToHost, st));
    MMT_HIP(hipStreamSynchronize(st));
    return total;
}

}  // namespace

uint64_t line_offsets(DevBuf<uint8_t>& temp, uint32_t* bytes, uint64_t* offset, size_t n, hipStream_t st) {
    MMT_HIP(hipMemsetAsync(bytes + n, 0, 4, st));
    prims::exclusive_sum_u32_to_u64(temp, bytes, offset, n + 1, st);
    return read_total(offset + n, st);
}
uint64_t line_offsets(DevBuf<uint8_t>& temp, uint64_t* bytes, uint64_t* offset, size_t n, hipStream_t st) {
    MMT_HIP(hipMemsetAsync(bytes + n, 0, 8, st));
    prims::exclusive_sum_u64(temp, bytes, offset, n + 1, st);
    return read_total(offset + n, st);
}

size_t text_piece_bytes(size_t dflt) {
    return sw::is_set(sw::MMT_MERGED_TEXT_PIECE) ? std::max<size_t>(sw::num(sw::MMT_MERGED_TEXT_PIECE, 0), 4096) : dflt;
}

double write_text_pieces(hipStream_t st, int device, const uint64_t* d_offset, size_t n, uint64_t bytes, size_t piece_bytes,
                         const std::string& path, const PieceFormat& format, PieceLaps laps) {
    using Clock = std::chrono::steady_clock;
    PieceCuts c;
    std::vector<uint64_t> h_off;
    const bool one = bytes <= piece_bytes;
    if (one) {
        c.cut.assign(1, 0);
        if (bytes) c.cut.push_back(n);
        c.longest = bytes;
    } else {
        d2h(h_off, d_offset, n + 1, st);
        c = cut_pieces(h_off.data(), n, piece_bytes);
    }
    DevBuf<char> d_piece[2];
    for (auto& d : d_piece) d.ensure((size_t)c.longest + 1);
    double wait_ms = 0;
    auto waited = [&wait_ms](Clock::time_point t0) { wait_ms += std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); };
    auto begin = [&laps](int stage) { const bool on = laps.laps && stage >= 0; if (on) laps.laps->begin(stage); return on; };
    auto end = [&laps](bool on) { if (on) laps.laps->end(); };
    PieceWriter writer((size_t)c.longest + 1, 2);
    writer.open(path, device, false);            // (left open by an exception: its destructor removes PATH.tmp)
    for (size_t i = 0; i + 1 < c.cut.size(); i++) {
        DevBuf<char>& d = d_piece[i & 1];
        const size_t k0 = c.cut[i], k1 = c.cut[i + 1];
        const uint64_t from = one ? 0 : h_off[k0], to = one ? bytes : h_off[k1];
        const auto t0 = Clock::now();
        PieceWriter::Piece pc = writer.room((size_t)(to - from));
        waited(t0);
        bool on = begin(laps.format);
        format(k0, k1, from, d.get());
        end(on);
        on = begin(laps.copy);
        MMT_HIP(hipMemcpyAsync(pc.p, d.get(), pc.n, hipMemcpyDeviceToHost, st));
        end(on);
        MMT_HIP(hipStreamSynchronize(st));
        writer.push(pc);
    }
    MMT_HIP(hipStreamSynchronize(st));
    if (laps.laps) laps.laps->collect();
    const auto t0 = Clock::now();
    writer.close();
    waited(t0);
    return wait_ms;
}

}  // namespace mmt
