// Driver (ours) around the REFERENCE's match scan: include/mem_finder.hpp fed by include/read_arrays.hpp
// (file_lcp, the reader of the CLI's `-a PREFIX` checkpoint), compiled from the reference tree by
// oracle/Makefile into oracle/_ref/mem_finder_ref.  The sdsl names those headers mention come from our
// own declarations in sdsl_shim/ (the scan uses only doc_ends_rank, a binary search there).
//
// Usage: mem_finder_ref ARRAYS OUT min_len num_distinct max_doc_freq max_total_freq revcomp binary merge anchor_merge
//   ARRAYS.sa / ARRAYS.lcp  40-bit little-endian entries, ARRAYS.bwt one byte per entry (the `-a` format);
//   ARRAYS.doclens          one line per document: its length in the text (F '$' [revcomp '$']).
// Every entry of the files is streamed (RefBuilder::total_length = entries in the file, not |T|), so a
// prefix of the stream over a text of any length is legal input.  Writes whatever mem_finder::close()
// writes under OUT: .mums | .mems | .bumbl, and .thresh / .thresh_rev | .athresh.
//
// Binary mode: mem_finder::write_bums (mem_finder.hpp:460-463) reads bums_strands_vec[0] to learn the
// number of documents, so a .bumbl run that finds no MUM at all reads past an empty vector and crashes
// in the reference itself.  The driver refuses that case (exit 3) instead of running it; .bumbl keeps
// its check against the reference's Python writer (tests/test_oracle.py).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <unordered_map>
#include <vector>

#define PBWIDTH 60
static void printProgress(double) {}            // file_lcp::process reports progress; the driver stays quiet

#include <ref_builder.hpp>
#include <read_arrays.hpp>
#include <mem_finder.hpp>

// The one RefBuilder constructor the driver needs; the public fields are filled in main().
RefBuilder::RefBuilder(std::string output_prefix, bool use_rcomp) : use_revcomp(use_rcomp), output_prefix(output_prefix) {}

// mem_finder unchanged; the subclass only reads how many .bumbl rows were collected, so that an empty
// binary run can be refused before close() (see the header comment).
struct counted_mem_finder : mem_finder {
    using mem_finder::mem_finder;
    size_t binary_rows() const { return bums_strands_vec.size(); }
};

int main(int argc, char** argv) {
    if (argc != 11) {
        std::fprintf(stderr, "usage: %s ARRAYS OUT min_len num_distinct max_doc_freq max_total_freq revcomp binary merge "
                             "anchor_merge\n", argv[0]);
        return 2;
    }
    const std::string arrays = argv[1], out = argv[2];
    const size_t min_len = std::strtoull(argv[3], nullptr, 10), num_distinct = std::strtoull(argv[4], nullptr, 10);
    const int max_doc_freq = std::atoi(argv[5]), max_total_freq = std::atoi(argv[6]);
    const bool revcomp = std::atoi(argv[7]) != 0, binary = std::atoi(argv[8]) != 0, merge = std::atoi(argv[9]) != 0,
               anchor = std::atoi(argv[10]) != 0;

    RefBuilder ref(out, revcomp);
    {
        std::ifstream in(arrays + ".doclens");
        uint64_t len;
        while (in >> len) ref.seq_lengths.push_back(len);
    }
    if (ref.seq_lengths.empty()) { std::fprintf(stderr, "no document lengths in %s.doclens\n", arrays.c_str()); return 2; }
    ref.num_docs = ref.seq_lengths.size();
    uint64_t end = 0;
    for (uint64_t len : ref.seq_lengths) { end += len; ref.doc_ends_rank.ends.push_back(end - 1); }
    {
        std::ifstream sa(arrays + ".sa", std::ios::binary | std::ios::ate), bwt(arrays + ".bwt", std::ios::binary | std::ios::ate),
            lcp(arrays + ".lcp", std::ios::binary | std::ios::ate);
        const uint64_t e = (uint64_t)sa.tellg() / 5;
        if (!sa || !bwt || !lcp || (uint64_t)lcp.tellg() != 5 * e || (uint64_t)bwt.tellg() != e || (uint64_t)sa.tellg() != 5 * e) {
            std::fprintf(stderr, "%s.sa / .lcp / .bwt missing or of unequal entry counts\n", arrays.c_str());
            return 2;
        }
        ref.total_length = e;
    }

    file_lcp input(arrays, &ref);
    counted_mem_finder finder(out, ref, min_len, num_distinct, max_doc_freq, max_total_freq, binary, merge, anchor);
    const size_t found = input.process(finder);
    input.close();
    (void)found;                                  // process() sums into an uninitialised counter (read_arrays.hpp:74)
    if (binary && finder.binary_rows() == 0) {
        std::fprintf(stderr, "binary mode without any MUM: the reference's write_bums would index an empty vector\n");
        return 3;
    }
    finder.close();
    return 0;
}
