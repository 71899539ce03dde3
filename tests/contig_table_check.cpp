// contig_table_check.cpp -- check_contig_table (mumemto_amd/csrc/contig_table.cpp) as a stand-alone program for the host
// sanitizers (tests/test_contig_table_host.py builds and runs it).
//   contig_table_check CASES   every line of CASES is
//       who;first;last;n_docs;use_names;contig_begin;contig_len;name_begin;names;end
//   who is bed or label (and stands for what bed() and label() pass: names required / optional, the forbidden bytes, what a
//   sequence holds), the three arrays are numbers separated by commas, names is hexadecimal, and - is a null pointer.  Per
//   line it prints "refused;MESSAGE" or "ok;n_contigs;name_bytes;ends;totals;longest_name".
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "contig_table.cpp"

template <typename T>
static bool numbers(const std::string& field, std::vector<T>& out) {      // false: a null pointer
    out.clear();
    if (field == "-") return false;
    std::istringstream ss(field);
    std::string tok;
    while (std::getline(ss, tok, ',')) out.push_back((T)std::stoll(tok));
    return true;
}
template <typename T>
static std::string joined(const std::vector<T>& v) {
    std::string s;
    for (size_t i = 0; i < v.size(); i++) s += (i ? "," : "") + std::to_string(v[i]);
    return s;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: contig_table_check CASES\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::vector<std::string> f;
        std::istringstream ss(line);
        for (std::string tok; std::getline(ss, tok, ';');) f.push_back(tok);
        if (f.size() != 10) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
        const bool label = f[0] == "label";
        const mmt::ContigSpec spec{f[0].c_str(), (uint32_t)std::stoul(f[1]), (uint32_t)std::stoul(f[2]), label,
                                   label ? f[4] == "1" : true, label ? "\t\n," : "\t\n", label ? "a start" : "an interval"};
        // (vectors of exactly the given sizes: a read beyond them is the sanitizer's)
        std::vector<uint64_t> begin, name_begin;
        std::vector<int64_t> len;
        std::vector<char> names;
        const bool has_begin = numbers(f[5], begin), has_len = numbers(f[6], len), has_nb = numbers(f[7], name_begin);
        const bool has_names = f[8] != "-";
        for (size_t i = 0; has_names && i + 1 < f[8].size(); i += 2) names.push_back((char)std::stoi(f[8].substr(i, 2), nullptr, 16));
        try {
            const mmt::ContigTable t = mmt::check_contig_table(spec, (uint32_t)std::stoul(f[3]), has_begin ? begin.data() : nullptr,
                                                               has_len ? len.data() : nullptr, has_nb ? name_begin.data() : nullptr,
                                                               has_names ? names.data() : nullptr);
            std::printf("ok;%llu;%llu;%s;%s;%s\n", (unsigned long long)t.n_contigs, (unsigned long long)t.name_bytes,
                        joined(t.ends).c_str(), joined(t.totals).c_str(), joined(t.longest_name).c_str());
        } catch (const std::invalid_argument& e) {
            std::string msg = e.what();
            for (char& ch : msg) if (ch == '\n') ch = ' ';
            std::printf("refused;%s\n", msg.c_str());
        }
    }
    return 0;
}
