// contig_table.cpp -- see contig_table.hpp.
#include "contig_table.hpp"

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>

namespace mmt {
namespace {

// "a tab or a newline", "a tab, a newline or a comma"
std::string spell(const char* forbidden) {
    std::string out;
    const size_t k = std::strlen(forbidden);
    for (size_t i = 0; i < k; i++) {
        if (i) out += i + 1 == k ? " or " : ", ";
        out += forbidden[i] == '\t' ? "a tab" : forbidden[i] == '\n' ? "a newline" : "a comma";
    }
    return out;
}

}  // namespace

ContigTable check_contig_table(const ContigSpec& spec, uint32_t n_docs, const uint64_t* contig_begin, const int64_t* contig_len,
                               const uint64_t* name_begin, const char* names) {
    const std::string who = std::string(spec.who) + ": ";
    auto refuse = [&](const std::string& what) { throw std::invalid_argument(who + what); };
    auto seq = [](uint32_t c) { return "sequence " + std::to_string(c); };
    if (!contig_begin) refuse("contig_begin must hold n_docs + 1 entries");
    for (uint32_t c = 0; c < n_docs; c++)
        if (contig_begin[c] > contig_begin[c + 1]) refuse("contig_begin does not ascend");
    ContigTable t;
    t.n_contigs = contig_begin[n_docs];
    if (spec.names_optional) {
        if (t.n_contigs && !contig_len) refuse("contig_len must hold an entry per contig");
        if (spec.use_names && !name_begin) refuse("name_begin must hold an entry per contig and one more");
    } else if (t.n_contigs && (!contig_len || !name_begin)) {
        refuse("contig_len and name_begin must hold an entry per contig (name_begin one more)");
    }
    if (spec.use_names) {
        for (uint64_t g = 0; g < t.n_contigs; g++)
            if (name_begin[g] > name_begin[g + 1]) refuse("name_begin does not ascend");
        t.name_bytes = t.n_contigs ? name_begin[t.n_contigs] : 0;
        if (t.name_bytes && !names) refuse("names must hold the bytes name_begin refers to");
    }
    // cumulative lengths per column; the needed columns are checked
    t.ends.assign((size_t)t.n_contigs + 1, 0);
    t.totals.assign(n_docs, 0);
    t.longest_name.assign(n_docs, 0);
    for (uint32_t c = 0; c < n_docs; c++) {
        const bool needed = c >= spec.first && c < spec.last;
        if (needed && contig_begin[c] == contig_begin[c + 1]) refuse(seq(c) + " has no contigs");
        uint64_t run = 0;
        for (uint64_t g = contig_begin[c]; g < contig_begin[c + 1]; g++) {
            auto contig = [&] { return "contig " + std::to_string(g - contig_begin[c]) + " of " + seq(c); };
            if (needed && contig_len[g] < 0) refuse(contig() + " has the negative length " + std::to_string(contig_len[g]));
            run += (uint64_t)contig_len[g];
            if (needed && run >> 62) refuse(seq(c) + " is 2^62 bases or longer");
            t.ends[g] = (int64_t)run;
            if (!needed || !spec.use_names) continue;
            t.longest_name[c] = std::max<uint64_t>(t.longest_name[c], name_begin[g + 1] - name_begin[g]);
            for (uint64_t i = name_begin[g]; i < name_begin[g + 1]; i++)
                if (names[i] && std::strchr(spec.forbidden, names[i]))
                    refuse("the name of " + contig() + " contains " + spell(spec.forbidden));
        }
        if (needed && run == 0) refuse(seq(c) + " has total length 0: no contig can hold " + spec.holds);
        t.totals[c] = (int64_t)run;
    }
    return t;
}

}  // namespace mmt
