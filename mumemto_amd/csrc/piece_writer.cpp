// piece_writer.cpp -- the helper thread and the ring of page-locked blocks behind PieceWriter.
#include "piece_writer.hpp"

namespace mmt {

void PieceWriter::open(const std::string& path, int device, bool digest, Early early) {
    close(false);
    file_.open(path);
    want_digest_ = digest || file_.special();
    digest_ = StreamDigest(); written_ = 0; digest_value_ = 0; block_at_ = 0; block_used_ = 0;
    block_pending_.assign(blocks_.size(), 0);
    closing_ = false; error_.clear();
    stats_ = Stats();
    // the blocks an output of the expected size will fill, one or two: one is filled while the other is written, and a
    // caller that gets ahead of the helper asks for the rest of the ring (room())
    const size_t eager = (size_t)std::min<uint64_t>(std::min<size_t>(ring_, 2), (early.expected_bytes + block_bytes_ - 1) / std::max<size_t>(block_bytes_, 1));
    ring_wanted_ = early.expected_bytes ? std::max<size_t>(eager, 1) : 0;
    ring_needed_ = 0;
    const bool retire_old = early.retire_old;
    active_ = true;
    thread_ = std::thread([this, device, retire_old]() { run(device, retire_old); });
}

void PieceWriter::run(int device, bool retire_old) {
    (void)hipSetDevice(device);
    auto fail_with = [&](const std::string& what) { std::lock_guard<std::mutex> lk(mu_); if (error_.empty()) error_ = what; };
    for (;;) {
        Piece pc;
        enum { BLOCK, PIECE, RETIRE } what;
        {
            std::unique_lock<std::mutex> lk(mu_);
            for (;;) {
                if (q_.empty() && closing_) return;
                const bool ok = error_.empty() && !closing_;
                // a block the caller is blocked for goes before a piece, a piece before a block it only will want
                if (ok && blocks_.size() < ring_needed_) { what = BLOCK; break; }
                if (!q_.empty()) { pc = q_.front(); q_.pop_front(); what = PIECE; break; }
                if (ok && blocks_.size() < ring_wanted_) { what = BLOCK; break; }
                if (ok && retire_old) { what = RETIRE; break; }
                const auto t0 = Clock::now();
                cv_.wait(lk, [&] { return !q_.empty() || closing_ || (error_.empty() && blocks_.size() < std::max(ring_needed_, ring_wanted_)); });
                stats_.wait_queue_s += since(t0);
            }
        }
        if (what == BLOCK) {
            const auto t0 = Clock::now();
            std::unique_ptr<PinnedBuf<char>> block(new PinnedBuf<char>());
            try { block->ensure(block_bytes_); } catch (const std::exception& e) { fail_with(e.what()); }
            stats_.ring_s += since(t0); stats_.blocks_made++;
            {
                std::lock_guard<std::mutex> lk(mu_);
                if (error_.empty()) { blocks_.push_back(std::move(block)); block_cap_.push_back(block_bytes_); block_pending_.push_back(0); }
            }
            cv_.notify_all();
            continue;
        }
        if (what == RETIRE) {
            const auto t0 = Clock::now();
            file_.retire_old();
            stats_.retire_s += since(t0);
            retire_old = false;
            continue;
        }
        if (pc.ready) {
            const auto t0 = Clock::now();
            if (hipEventSynchronize(pc.ready) != hipSuccess) fail_with("device copy of the output failed");
            (void)hipEventDestroy(pc.ready);
            stats_.wait_event_s += since(t0);
        }
        // this one thread writes the pieces in order; whole words are carried across piece boundaries, which fall where
        // windows end and differ from box to box.  After a failure pieces are only counted off: their memory may be gone.
        if (!failed()) {
            const auto t0 = Clock::now();
            const bool wrote = file_.write_all(pc.p, pc.n);
            stats_.write_s += since(t0);
            if (!wrote) fail_with(file_.error());
            else {
                if (want_digest_) digest_.update(pc.p, pc.n);
                written_ += pc.n;
                stats_.pieces++;
            }
        }
        { std::lock_guard<std::mutex> lk(mu_); block_pending_[pc.block]--; }
        cv_.notify_all();
    }
}

PieceWriter::Piece PieceWriter::room(size_t n) {
    const size_t want = std::max(block_bytes_, n);
    std::unique_lock<std::mutex> lk(mu_);
    if (!error_.empty()) throw std::runtime_error(error_);
    if (block_at_ >= blocks_.size() || block_used_ + n > block_cap_[block_at_]) {
        // the next block: one whose pieces are all written, the oldest first -- a writer that keeps up with its caller never
        // page-locks the whole ring; otherwise a new one while the ring is short (the helper makes it); otherwise the oldest,
        // once it is written
        size_t next = blocks_.size();
        for (size_t k = 1; k <= blocks_.size() && next == blocks_.size(); k++) {
            const size_t b = (block_at_ + k) % blocks_.size();
            if (block_pending_[b] == 0) next = b;
        }
        if (next >= ring_) next = (block_at_ + 1) % blocks_.size();
        if (next >= blocks_.size()) {
            ring_needed_ = std::max(ring_needed_, next + 1);
            cv_.notify_all();
            const auto t0 = Clock::now();
            cv_.wait(lk, [&] { return next < blocks_.size() || !error_.empty(); });
            stats_.room_create_s += since(t0);
            if (!error_.empty()) throw std::runtime_error(error_);
        }
        if (block_pending_[next] != 0) {
            const auto t0 = Clock::now();
            cv_.wait(lk, [&] { return block_pending_[next] == 0 || !error_.empty(); });
            stats_.room_wait_s += since(t0);
        }
        if (!error_.empty()) throw std::runtime_error(error_);
        if (block_cap_[next] < want) {
            // a piece larger than a block gets a block of its size (nobody reads an idle block)
            PinnedBuf<char>* block = blocks_[next].get();
            const auto t0 = Clock::now();
            lk.unlock(); block->ensure(want); lk.lock();
            stats_.room_create_s += since(t0);
            block_cap_[next] = want;
        }
        block_at_ = next; block_used_ = 0;
    }
    Piece pc;
    pc.p = blocks_[block_at_]->get() + block_used_; pc.n = n; pc.block = (uint32_t)block_at_;
    block_used_ += n; block_pending_[block_at_]++;
    return pc;
}

void PieceWriter::close(bool ok) {
    if (!active_) return;
    { std::lock_guard<std::mutex> lk(mu_); closing_ = true; }
    cv_.notify_all();
    auto t0 = Clock::now();
    thread_.join();
    stats_.join_s = since(t0);
    active_ = false;
    stats_.bytes = file_.written();
    std::string error;
    { std::lock_guard<std::mutex> lk(mu_); error = error_; }
    if (error.empty() && !ok) error = "the run failed";
    if (!error.empty()) { file_.abort(); throw std::runtime_error(error); }
    t0 = Clock::now();
    file_.commit();
    stats_.commit_s = since(t0);
    digest_value_ = digest_.final();
    if (sw::on(sw::MUMEMTO_TIMING)) print_stats("piece writer");
}

void PieceWriter::print_stats(const char* who) const {
    const Stats& s = stats_;
    std::fprintf(stderr, "[%s] %llu bytes in %llu pieces | helper: write %.1f ms, queue empty %.1f, copy event %.1f, blocks %.1f (%llu made), "
                         "earlier file %.1f | caller: room for a written block %.1f ms, for a new block %.1f, join %.1f, commit %.1f\n",
                 who, (unsigned long long)s.bytes, (unsigned long long)s.pieces, s.write_s * 1e3, s.wait_queue_s * 1e3, s.wait_event_s * 1e3,
                 s.ring_s * 1e3, (unsigned long long)s.blocks_made, s.retire_s * 1e3, s.room_wait_s * 1e3, s.room_create_s * 1e3,
                 s.join_s * 1e3, s.commit_s * 1e3);
}

}  // namespace mmt
