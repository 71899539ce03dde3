// out_file.hpp -- one output file of the library: its name while it is written, the write loop, the error strings.
// Host code only (extract_mums is built without the device toolchain).
#pragma once
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

namespace mmt {

// digest of a byte stream that arrives in pieces of any size (the text sink's bytes in file order)
struct StreamDigest {
    uint64_t h = 0x6d756d656d746f35ull;
    uint8_t carry[8];
    uint32_t have = 0;
    void word(uint64_t w) { h = (h ^ w) * 0x9E3779B97F4A7C15ull; h ^= h >> 29; }
    void update(const char* p, size_t n) {
        size_t i = 0;
        while (have && have < 8 && i < n) carry[have++] = (uint8_t)p[i++];
        if (have == 8) { uint64_t w; std::memcpy(&w, carry, 8); word(w); have = 0; }
        for (; i + 8 <= n; i += 8) { uint64_t w; std::memcpy(&w, p + i, 8); word(w); }
        for (; i < n; i++) carry[have++] = (uint8_t)p[i];
    }
    uint64_t final() const { uint64_t x = h; for (uint32_t i = 0; i < have; i++) x = (x ^ carry[i]) * 0x100000001b3ull; return x ^ (x >> 31); }
};

// The bytes go to PATH.tmp and take the final name in commit(): a run that fails half way -- a short write, a full disk, a
// consistency check at its end -- must not leave a plausible but truncated PATH.  A path that exists and is not a regular
// file (a FIFO, /dev/stdout) and "/dev/null" are written as they are; IN_PLACE writes any path under its own name.
//
// A PATH left by an earlier run is replaced by the rename -- and the file system frees its pages inside that call, the last
// one before the run is over (~0.09 s per GB of a file in memory).  A writer that has idle time before its bytes arrive
// calls retire_old() then: the old PATH goes at once, as with a tool that opens its output for writing when it starts,
// and a run that fails afterwards leaves no PATH at all.
class OutFile {
public:
    enum Mode { RENAME, IN_PLACE };
    OutFile() = default;
    OutFile(const OutFile&) = delete;
    ~OutFile() { abort(); }
    void open(const std::string& path, Mode mode = RENAME) {
        abort();                    // (a file left open is dropped, PATH.tmp with it)
        struct stat sb;
        special_ = path == "/dev/null" || (::stat(path.c_str(), &sb) == 0 && !S_ISREG(sb.st_mode));
        rename_ = mode == RENAME && !special_;
        path_ = path; name_ = rename_ ? path + ".tmp" : path; error_.clear(); written_ = 0;
        fd_ = ::open(name_.c_str(), special_ ? O_WRONLY : (O_CREAT | O_TRUNC | O_WRONLY), 0644);
        if (fd_ < 0) throw std::runtime_error("cannot write " + name_);
    }
    // removes what an earlier run left under the final name (RENAME mode; nothing to do for the other files)
    void retire_old() { if (rename_) ::unlink(path_.c_str()); }
    // false once a write has failed (the first failure stays in error(); later calls write nothing)
    bool write_all(const void* data, size_t n) {
        const char* src = static_cast<const char*>(data);
        for (size_t at = 0; error_.empty() && at < n;) {
            const ssize_t w = ::write(fd_, src + at, std::min<size_t>(n - at, (size_t)1 << 30));
            if (w <= 0) error_ = "short write to " + name_;
            else { at += (size_t)w; written_ += (uint64_t)w; }
        }
        return error_.empty();
    }
    // closes the file and gives it its name; throws what went wrong since open() after removing PATH.tmp
    void commit() {
        if (fd_ >= 0 && ::close(fd_) != 0 && error_.empty()) error_ = "cannot close " + name_;
        fd_ = -1;
        if (error_.empty() && rename_ && std::rename(name_.c_str(), path_.c_str()) != 0) error_ = "cannot rename " + name_;
        if (!error_.empty()) { abort(); throw std::runtime_error(error_); }
        rename_ = false;
    }
    void abort() noexcept {
        if (fd_ >= 0) ::close(fd_);
        if (rename_) ::unlink(name_.c_str());
        fd_ = -1; rename_ = false;
    }
    bool special() const { return special_; }       // not a regular file: nobody can read the bytes back
    const std::string& error() const { return error_; }
    uint64_t written() const { return written_; }

private:
    std::string path_, name_, error_;
    int fd_ = -1;
    bool special_ = false, rename_ = false;
    uint64_t written_ = 0;
};

}  // namespace mmt
