// piece_writer.hpp -- bytes that leave the device in pieces, written to one file by a helper thread meanwhile.
#pragma once
#include <chrono>
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
// every piece in it has been written, and a new one is made only when none is free: at most `ring` blocks however large the
// output is (a larger piece gets a block of its size).
//
// The helper thread does everything that is not the caller's business, in this order of urgency: it page-locks a block the
// caller is blocked for, it writes the queued pieces in order, and while it has nothing to write it prepares what the caller
// will want (Early): it removes the file an earlier run left under the final name and page-locks the blocks an output of the
// expected size will fill (~0.19 s per GB).  What each side spent where is counted (Stats): the instrument behind DESIGN.md
// section 7.
class PieceWriter {
public:
    // page-locked room for n bytes; ready: the copy into it has landed (destroyed by the writer; none: it has already)
    struct Piece { char* p = nullptr; size_t n = 0; uint32_t block = 0; hipEvent_t ready = nullptr; };

    // What the caller knows when it opens the file long before its first piece.  expected_bytes: an estimate of the output
    // (0: none) -- the blocks it will fill, one or two, are page-locked right away, the others when room() asks for them.
    // retire_old: what an earlier run left under the final name goes right away as well (OutFile::retire_old).
    struct Early { uint64_t expected_bytes = 0; bool retire_old = false; };

    // seconds by the host clock, of the last file (reset by open())
    struct Stats {
        uint64_t bytes = 0, pieces = 0;
        double write_s = 0;                           // helper: inside OutFile::write_all
        double wait_queue_s = 0, wait_event_s = 0;    // helper: nothing queued (and nothing else to do) / the copy of a queued piece
        double ring_s = 0, retire_s = 0;              // helper: page-locking blocks / removing the earlier run's file
        uint64_t blocks_made = 0;
        double room_wait_s = 0, room_create_s = 0;    // caller, blocked in room(): for a written block / for a block to exist (or grow)
        double join_s = 0, commit_s = 0;              // caller, in close(): the helper's last pieces / close, rename
    };

    PieceWriter(size_t block_bytes, size_t ring) : block_bytes_(block_bytes), ring_(ring) {}
    ~PieceWriter() { try { close(false); } catch (...) {} }
    PieceWriter(const PieceWriter&) = delete;

    // starts the helper thread; digest: keep a digest of the bytes in file order (always kept for a file nobody can read back)
    void open(const std::string& path, int device, bool digest, Early early);
    void open(const std::string& path, int device, bool digest) { open(path, device, digest, Early()); }
    bool active() const { return active_; }
    Piece room(size_t n);         // waits until the oldest block of a full ring is written; throws once a piece has failed
    void push(const Piece& pc) { { std::lock_guard<std::mutex> lk(mu_); q_.push_back(pc); } cv_.notify_all(); }
    // joins the thread; ok and no error: the file takes its name; otherwise it is removed and the first error thrown
    void close(bool ok = true);
    // both of the last file that was closed well: the helper thread alone counts while a file is open, ask after close()
    uint64_t written() const { return written_; }
    uint64_t digest() const { return digest_value_; }
    const Stats& stats() const { return stats_; }           // (after close())
    void print_stats(const char* who) const;                // one line on stderr (MUMEMTO_TIMING)

private:
    using Clock = std::chrono::steady_clock;
    static double since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }
    void run(int device, bool retire_old);
    bool failed() { std::lock_guard<std::mutex> lk(mu_); return !error_.empty(); }
    const size_t block_bytes_, ring_;
    OutFile file_;
    bool active_ = false, want_digest_ = false;
    StreamDigest digest_;
    uint64_t written_ = 0, digest_value_ = 0;
    Stats stats_;                          // the helper's and the caller's fields are disjoint; read after the join
    std::thread thread_;
    std::mutex mu_;                        // guards everything below
    std::condition_variable cv_;
    std::deque<Piece> q_;
    bool closing_ = false;
    std::string error_;                    // the first failure
    std::vector<std::unique_ptr<PinnedBuf<char>>> blocks_;      // grown by the helper alone, up to ring_
    std::vector<size_t> block_cap_;
    std::vector<uint32_t> block_pending_;  // pieces of a block the thread has not written yet
    size_t ring_wanted_ = 0;               // blocks an output of the expected size will want (at most ring_)
    size_t ring_needed_ = 0;               // blocks room() has asked for: the caller is blocked until they exist
    size_t block_at_ = 0, block_used_ = 0;
};

}  // namespace mmt
