// out_file_check.cpp -- OutFile (mumemto_amd/csrc/out_file.hpp) as a stand-alone program for the
// host sanitizers (tests/test_out_file_host.py builds and runs it).  Usage: out_file_check DIR; prints "out_file ok".
#include <sys/stat.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "out_file.hpp"

using mmt::OutFile;

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

static const size_t TOTAL = 10001;

static std::string payload() {
    std::string s(TOTAL, '\0');
    uint32_t x = 12345;
    for (char& c : s) { x = x * 1664525u + 1013904223u; c = (char)('A' + (x >> 24) % 26); }
    return s;
}
static long size_of(const std::string& path) { struct stat sb; return ::stat(path.c_str(), &sb) == 0 ? (long)sb.st_size : -1; }
static std::string slurp(const std::string& path) {
    std::ifstream in(path, std::ios::binary);
    return std::string(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
}

// the bytes [from, upto) in pieces of 1, 4095 and 4097 bytes in turn
static void write_pieces(OutFile& f, const std::string& data, size_t from, size_t upto) {
    const size_t sizes[3] = {1, 4095, 4097};
    size_t at = from;
    for (int k = 0; at < upto; k++) {
        const size_t n = std::min(sizes[k % 3], upto - at);
        CHECK(f.write_all(data.data() + at, n));
        at += n;
        CHECK(f.written() == at);
    }
}
static void put(const std::string& path, const std::string& bytes) { std::ofstream(path, std::ios::binary) << bytes; }

int main(int argc, char** argv) {
    CHECK(argc == 2);
    const std::string dir = argv[1], data = payload(), old = "the output of an earlier run\n";
    const std::string path = dir + "/out.txt", tmp = path + ".tmp";

    // commit: PATH.tmp until then, the exact bytes under PATH afterwards; an earlier PATH stays until the rename
    {
        put(path, old);
        OutFile f;
        f.open(path);
        write_pieces(f, data, 0, TOTAL);
        CHECK(size_of(tmp) == (long)TOTAL && slurp(path) == old);
        f.commit();
        CHECK(size_of(tmp) == -1 && size_of(path) == (long)TOTAL && slurp(path) == data);
    }
    // retire_old: the earlier PATH goes at once, the new one appears with the commit
    {
        CHECK(size_of(path) == (long)TOTAL);
        OutFile f;
        f.open(path);
        f.retire_old();
        CHECK(size_of(path) == -1 && size_of(tmp) == 0);
        f.retire_old();                             // (nothing there: nothing happens)
        write_pieces(f, data, 0, TOTAL);
        CHECK(size_of(path) == -1);
        f.commit();
        CHECK(size_of(tmp) == -1 && slurp(path) == data);
    }
    // abort, and a file that is dropped: nothing of this run is left; after retire_old nothing at all
    {
        OutFile f;
        f.open(path);
        write_pieces(f, data, 0, 5000);
        CHECK(size_of(tmp) == 5000);
        f.abort();
        CHECK(size_of(tmp) == -1 && slurp(path) == data);
        { OutFile g; g.open(path); g.retire_old(); write_pieces(g, data, 0, 5000); }
        CHECK(size_of(tmp) == -1 && size_of(path) == -1);
    }
    // IN_PLACE: written under the final name, retire_old leaves it alone, the file that is given up holds the bytes written
    {
        OutFile f;
        f.open(path, OutFile::IN_PLACE);
        f.retire_old();
        CHECK(size_of(path) == 0 && size_of(tmp) == -1);
        write_pieces(f, data, 0, 5000);
        f.abort();
        CHECK(size_of(path) == 5000 && slurp(path) == data.substr(0, 5000));
        f.open(path, OutFile::IN_PLACE);
        write_pieces(f, data, 0, TOTAL);
        f.commit();
        CHECK(size_of(path) == (long)TOTAL && slurp(path) == data);
        std::remove(path.c_str());
    }
    // a special file is written as it is
    {
        OutFile f;
        f.open("/dev/null");
        f.retire_old();
        CHECK(f.special() && size_of("/dev/null") == 0);
        write_pieces(f, data, 0, TOTAL);
        f.commit();
        CHECK(size_of("/dev/null") == 0);
    }
    // a write that fails: the first error stays, commit throws it and removes PATH.tmp
    {
        const std::string full = dir + "/full.txt";
        CHECK(::symlink("/dev/full", full.c_str()) == 0);
        OutFile f;
        f.open(full);
        CHECK(f.special() && !f.write_all(data.data(), 100) && f.error() == "short write to " + full);
        bool thrown = false;
        try { f.commit(); } catch (const std::runtime_error& e) { thrown = std::string(e.what()) == "short write to " + full; }
        CHECK(thrown);
        std::remove(full.c_str());
    }
    std::puts("out_file ok");
    return 0;
}
