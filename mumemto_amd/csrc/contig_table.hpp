// contig_table.hpp -- the contig tables a caller hands to bed() and label(), checked and summed on the host.  Plain C++: no
// device header, so that a host compiler alone builds it (tests/contig_table_check.cpp).
//
// The tables: contig_begin (n_docs + 1, ascending: the contigs of column c are [contig_begin[c], contig_begin[c + 1]) among
// all contigs), contig_len (per contig), name_begin (per contig and one more, ascending: the name of contig g is
// names[name_begin[g] .. name_begin[g + 1])).
#pragma once
#include <cstdint>
#include <vector>

namespace mmt {

struct ContigSpec {
    const char* who;            // the prefix of every message: "bed", "label"
    uint32_t first, last;       // the columns [first, last) are needed: only their contigs and names are checked
    bool names_optional;        // the caller works without names (label): name_begin and names are looked at only with use_names
    bool use_names;
    const char* forbidden;      // bytes no name of a needed column may hold: "\t\n", or "\t\n," where names are listed with commas
    const char* holds;          // what a sequence of total length 0 cannot hold: "an interval", "a start"
};

struct ContigTable {
    uint64_t n_contigs = 0, name_bytes = 0;       // name_bytes: 0 without names
    std::vector<int64_t> ends;                    // n_contigs + 1: per contig the cumulative length inside its column
    std::vector<int64_t> totals;                  // n_docs: the length of the column's sequence
    std::vector<uint64_t> longest_name;           // n_docs: 0 without names and for a column that is not needed
};

// throws std::invalid_argument with the message of the first fault
ContigTable check_contig_table(const ContigSpec& spec, uint32_t n_docs, const uint64_t* contig_begin, const int64_t* contig_len,
                               const uint64_t* name_begin, const char* names);

}  // namespace mmt
