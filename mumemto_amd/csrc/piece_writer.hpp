// piece_writer.hpp -- bytes that leave the device in pieces, written to one file by a helper thread meanwhile.
#pragma once
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "device_utils.hpp"
#include "out_file.hpp"

namespace mmt {

// Page-locked room for the pieces is a RING of blocks that stay with the writer between files.  A block is used again once
// every piece in it has been written: `ring` blocks however large the output is (a larger piece gets a block of its size).
class PieceWriter {
public:
    // page-locked room for n bytes; ready: the copy into it has landed (destroyed by the writer; none: it has already)
    struct Piece { char* p = nullptr; size_t n = 0; uint32_t block = 0; hipEvent_t ready = nullptr; };

    PieceWriter(size_t block_bytes, size_t ring) : block_bytes_(block_bytes), ring_(ring) {}
    ~PieceWriter() { try { close(false); } catch (...) {} }
    PieceWriter(const PieceWriter&) = delete;

    // starts the helper thread; digest: keep a digest of the bytes in file order (always kept for a file nobody can read back)
    void open(const std::string& path, int device, bool digest);
    bool active() const { return active_; }
    Piece room(size_t n);         // waits until the oldest block of a full ring is written; throws once a piece has failed
    void push(const Piece& pc) { { std::lock_guard<std::mutex> lk(mu_); q_.push_back(pc); } cv_.notify_all(); }
    // joins the thread; ok and no error: the file takes its name; otherwise it is removed and the first error thrown
    void close(bool ok = true);
    // both of the last file that was closed well: the helper thread alone counts while a file is open, ask after close()
    uint64_t written() const { return written_; }
    uint64_t digest() const { return digest_value_; }

private:
    void run(int device);
    bool failed() { std::lock_guard<std::mutex> lk(mu_); return !error_.empty(); }
    const size_t block_bytes_, ring_;
    OutFile file_;
    bool active_ = false, want_digest_ = false;
    StreamDigest digest_;
    uint64_t written_ = 0, digest_value_ = 0;
    std::thread thread_;
    std::mutex mu_;                        // guards everything below
    std::condition_variable cv_;
    std::deque<Piece> q_;
    bool closing_ = false;
    std::string error_;                    // the first failure
    std::vector<std::unique_ptr<PinnedBuf<char>>> blocks_;
    std::vector<size_t> block_cap_;
    std::vector<uint32_t> block_pending_;  // pieces of a block the thread has not written yet
    size_t block_at_ = 0, block_used_ = 0;
};

}  // namespace mmt
