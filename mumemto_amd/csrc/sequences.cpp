// sequences.cpp -- see sequences.hpp.  Stages: (1) measure: every row judged, the bytes of its record, where its bases begin, a
// 64-bit prefix sum -- kept with the table; (2) format, on demand: the records, whole or in pieces of whole records; (3) the
// bytes leave the device.
#include "sequences.hpp"

#include <stdexcept>
#include <string>
#include <vector>

#include "fasta.hpp"
#include "laps.hpp"
#include "sequence_kernels.hpp"
#include "text_pieces.hpp"

namespace mmt {
namespace {

sq::Format format_of(int dialect, bool terminator) {
    sq::Format f;
    const bool python = dialect == (int)SeqDialect::PYTHON;
    f.upper = f.strands = f.join = f.lenient = python ? 1 : 0;
    f.terminator = terminator ? 1 : 0;
    return f;
}

void check_sequences(const MergedRows& m) {
    if (!m.has_sequences) throw std::runtime_error("no sequences attached: call mmt_merged_sequences first");
}

// the text the sources of m point into
TextRef text_of(const Engine& e, const MergedRows& m) {
    if (m.seq_resident) {
        if (!e.have_text() || e.text_generation() != m.seq_text_generation || e.text_length() != m.seq_text_len)
            throw std::runtime_error("sequences: the engine's text is no longer the one the records were measured on");
        return e.text_ref();
    }
    TextRef T;
    T.v = m.d_seq_text.get() + Engine::TEXT_FRONT - 1;
    T.n = m.seq_text_len;
    return T;
}

// One document in TextRef's byte layout: a Dollar in front of the bases (TEXT_FRONT bytes of padding keep them 16-byte
// aligned), 32 Dollars and then zeros behind them.
void upload_document(MergedRows& m, const uint8_t* bases, uint64_t n, hipStream_t st) {
    std::vector<uint8_t> front(Engine::TEXT_FRONT, 0), back(Engine::TEXT_BACK, 0);
    front.back() = 2;
    for (size_t i = 0; i < 32; i++) back[i] = 2;
    m.d_seq_text.ensure(Engine::TEXT_FRONT + (size_t)n + Engine::TEXT_BACK);
    uint8_t* d = m.d_seq_text.get();
    MMT_HIP(hipMemcpyAsync(d, front.data(), front.size(), hipMemcpyHostToDevice, st));
    if (n) MMT_HIP(hipMemcpyAsync(d + Engine::TEXT_FRONT, bases, (size_t)n, hipMemcpyHostToDevice, st));
    MMT_HIP(hipMemcpyAsync(d + Engine::TEXT_FRONT + n, back.data(), back.size(), hipMemcpyHostToDevice, st));
    MMT_HIP(hipStreamSynchronize(st));           // (the host buffers are read until here)
}

void format_records(Engine& e, const MergedRows& m, const TextRef& T, size_t k0, size_t k1, uint64_t base, char* dst) {
    sq::format(T, m.d_seq_offset.get(), m.d_seq_source.get(), m.d_seq_bases.get(), (uint32_t)k0, (uint32_t)k1, (uint32_t)m.n_rows,
               base, m.seq_bytes, format_of(m.seq_dialect, m.seq_terminator), dst, e.stream());
}

}  // namespace

void sequences(Engine& e, MergedRows& m, const SeqSource& source, int64_t col, SeqDialect dialect, bool terminator,
               SequencesStats* stats) {
    m.has_sequences = false;                     // (a refused call leaves no sequences, those of an earlier call included)
    if (stats) *stats = SequencesStats();
    if (m.n_rows > 0xffffffffull)
        throw std::invalid_argument("sequences: a table of 2^32 rows or more (" + std::to_string(m.n_rows) + ") is not supported");
    if (col < 0 || col >= (int64_t)m.n_docs)
        throw std::invalid_argument("sequences: column " + std::to_string(col) + " is out of range (0-" +
                                    std::to_string((int64_t)m.n_docs - 1) + ")");
    if (dialect != SeqDialect::BINARY && dialect != SeqDialect::PYTHON)
        throw std::invalid_argument("sequences: unknown dialect " + std::to_string((int)dialect) + " (0 = binary, 1 = python)");
    uint64_t doc_begin = 0, doc_len = source.n;
    if (source.resident) {
        if (!e.have_text()) throw std::invalid_argument("sequences: the engine holds no text: run it first, or hand the document over");
        if (m.n_docs != e.n_docs())
            throw std::invalid_argument("sequences: the table has " + std::to_string(m.n_docs) + " columns, the engine's text " +
                                        std::to_string(e.n_docs()) + " documents");
        doc_begin = e.doc_start()[(size_t)col];
        doc_len = e.doc_len()[(size_t)col];
    } else if (!source.bases && source.n) {
        throw std::invalid_argument("sequences: null bases for a document of " + std::to_string(source.n) + " bases");
    }
    hipStream_t st = e.stream();
    MMT_HIP(hipSetDevice(e.device()));
    SequencesStats local;
    SequencesStats& S = stats ? *stats : local;
    Laps laps(st, stats ? S.ms : nullptr);
    const size_t n = m.n_rows;
    const sq::Format f = format_of((int)dialect, terminator);

    if (!source.resident) upload_document(m, source.bases, source.n, st);
    else m.d_seq_text.release();
    DevBuf<uint64_t> bytes, flags;
    flags.ensure(sq::N_FLAGS);
    bytes.ensure(n + 1); m.d_seq_offset.ensure(n + 1); m.d_seq_source.ensure(n + 1); m.d_seq_bases.ensure(n + 1);
    uint64_t total = 0, h_flags[sq::N_FLAGS];
    laps.begin(0);
    sq::clear_flags(flags.get(), st);
    sq::measure(m.d_offsets.get(), m.d_strands.get(), m.d_length.get(), (uint32_t)n, (uint32_t)m.n_docs, (uint32_t)col, doc_begin,
                doc_len, f, bytes.get(), m.d_seq_source.get(), m.d_seq_bases.get(), flags.get(), st);
    if (n) total = line_offsets(e.scratch(), bytes.get(), m.d_seq_offset.get(), n, st);
    else MMT_HIP(hipMemsetAsync(m.d_seq_offset.get(), 0, 8, st));
    laps.end();
    MMT_HIP(hipMemcpyAsync(h_flags, flags.get(), sizeof(h_flags), hipMemcpyDeviceToHost, st));
    MMT_HIP(hipStreamSynchronize(st));
    laps.collect();

    auto start_of = [&](uint64_t row) {
        int64_t s = 0;
        MMT_HIP(hipMemcpyAsync(&s, m.d_offsets.get() + row * m.n_docs + (size_t)col, 8, hipMemcpyDeviceToHost, st));
        MMT_HIP(hipStreamSynchronize(st));
        return s;
    };
    auto where = [&](uint64_t row) { return " of row " + std::to_string(row) + ", column " + std::to_string(col); };
    if (h_flags[sq::BAD_START] != sq::NO_ROW)
        throw std::invalid_argument("sequences: the start " + std::to_string(start_of(h_flags[sq::BAD_START])) +
                                    where(h_flags[sq::BAD_START]) + " lies below -1");
    if (h_flags[sq::PARTIAL] != sq::NO_ROW)
        throw std::invalid_argument("sequences: row " + std::to_string(h_flags[sq::PARTIAL]) + " has no start in column " +
                                    std::to_string(col) + " (a partial multi-MUM)");
    if (h_flags[sq::BEYOND] != sq::NO_ROW)
        throw std::invalid_argument("sequences: the start " + std::to_string(start_of(h_flags[sq::BEYOND])) + where(h_flags[sq::BEYOND]) +
                                    " lies beyond the document's end (" + std::to_string(doc_len) + " bases)");
    S.records = n;
    S.bases = h_flags[sq::BASES]; S.clipped = h_flags[sq::CLIPPED]; S.empty = h_flags[sq::EMPTY];
    S.text_bytes = total;
    m.seq_resident = source.resident;
    m.seq_terminator = terminator;
    m.seq_dialect = (int)dialect;
    m.seq_text_len = source.resident ? e.text_length() : source.n;
    m.seq_bytes = total;
    m.seq_text_generation = e.text_generation();
    m.has_sequences = true;
}

void sequences_file(Engine& e, MergedRows& m, const std::string& fasta, int64_t col, SeqDialect dialect, bool terminator,
                    SequencesStats* stats, uint64_t* doc_len) {
    m.has_sequences = false;
    std::vector<uint8_t> bases;
    read_fasta(fasta, bases);
    if (doc_len) *doc_len = bases.size();
    SeqSource source;
    source.resident = false; source.bases = bases.data(); source.n = bases.size();
    sequences(e, m, source, col, dialect, terminator, stats);
}

std::string sequences_text(Engine& e, const MergedRows& m, SequencesStats* stats) {
    check_sequences(m);
    const TextRef T = text_of(e, m);
    hipStream_t st = e.stream();
    MMT_HIP(hipSetDevice(e.device()));
    Laps laps(st, stats ? stats->ms : nullptr);
    const uint64_t bytes = m.seq_bytes;
    std::string out((size_t)bytes, '\0');
    if (bytes) {
        DevBuf<char> text;
        text.ensure((size_t)bytes + 1);
        laps.begin(1);
        format_records(e, m, T, 0, m.n_rows, 0, text.get());
        laps.end();
        MMT_HIP(hipMemcpyAsync(&out[0], text.get(), (size_t)bytes, hipMemcpyDeviceToHost, st));
        MMT_HIP(hipStreamSynchronize(st));
        laps.collect();
        if (stats) stats->pieces++;
    }
    return out;
}

// pieces of whole records, each at most this many bytes (a single longer record is a piece of its own); MMT_MERGED_TEXT_PIECE sets it
static constexpr size_t SEQUENCES_TEXT_PIECE = (size_t)256 << 20;

void sequences_write_text(Engine& e, const MergedRows& m, const std::string& path, SequencesStats* stats) {
    check_sequences(m);
    const TextRef T = text_of(e, m);
    hipStream_t st = e.stream();
    MMT_HIP(hipSetDevice(e.device()));
    Laps laps(st, stats ? stats->ms : nullptr);
    uint64_t pieces = 0;
    write_text_pieces(st, e.device(), m.d_seq_offset.get(), m.n_rows, m.seq_bytes, text_piece_bytes(SEQUENCES_TEXT_PIECE), path,
                      [&](size_t k0, size_t k1, uint64_t base, char* dst) {
                          format_records(e, m, T, k0, k1, base, dst);
                          pieces++;
                      },
                      {&laps, 1, -1});
    if (stats) stats->pieces += pieces;
}

}  // namespace mmt
