// piece_writer.cpp -- the helper thread and the ring of page-locked blocks behind PieceWriter.
#include "piece_writer.hpp"

namespace mmt {

void PieceWriter::open(const std::string& path, int device, bool digest) {
    close(false);
    file_.open(path);
    want_digest_ = digest || file_.special();
    digest_ = StreamDigest(); written_ = 0; digest_value_ = 0; block_at_ = 0; block_used_ = 0;
    block_pending_.assign(blocks_.size(), 0);
    closing_ = false; error_.clear();
    active_ = true;
    thread_ = std::thread([this, device]() { run(device); });
}

void PieceWriter::run(int device) {
    (void)hipSetDevice(device);
    for (;;) {
        Piece pc;
        {
            std::unique_lock<std::mutex> lk(mu_);
            cv_.wait(lk, [&] { return !q_.empty() || closing_; });
            if (q_.empty()) break;
            pc = q_.front(); q_.pop_front();
        }
        auto fail_with = [&](const std::string& what) { std::lock_guard<std::mutex> lk(mu_); if (error_.empty()) error_ = what; };
        if (pc.ready) {
            if (hipEventSynchronize(pc.ready) != hipSuccess) fail_with("device copy of the output failed");
            (void)hipEventDestroy(pc.ready);
        }
        // this one thread writes the pieces in order; whole words are carried across piece boundaries, which fall where
        // windows end and differ from box to box.  After a failure pieces are only counted off: their memory may be gone.
        if (!failed()) {
            if (!file_.write_all(pc.p, pc.n)) fail_with(file_.error());
            else { if (want_digest_) digest_.update(pc.p, pc.n); written_ += pc.n; }
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
        // the next block of the ring: a new one while the ring is short, otherwise the oldest, once it has been written
        size_t next = blocks_.size();
        if (next < ring_) {
            blocks_.emplace_back(new PinnedBuf<char>()); block_cap_.push_back(0); block_pending_.push_back(0);
        } else {
            next = (block_at_ + 1) % blocks_.size();
            cv_.wait(lk, [&] { return block_pending_[next] == 0 || !error_.empty(); });
            if (!error_.empty()) throw std::runtime_error(error_);
        }
        if (block_cap_[next] < want) {
            lk.unlock(); blocks_[next]->ensure(want); lk.lock();      // (nobody reads an idle block)
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
    thread_.join();
    active_ = false;
    std::string error;
    { std::lock_guard<std::mutex> lk(mu_); error = error_; }
    if (error.empty() && !ok) error = "the run failed";
    if (!error.empty()) { file_.abort(); throw std::runtime_error(error); }
    file_.commit();
    digest_value_ = digest_.final();
}

}  // namespace mmt
