// Bounded read-ahead of a frame series on a helper thread (--batch_frames): the reader keeps up to `ahead` frames
// read past the newest frame taken; take(k) hands frame k over (any order) and reads it again through the source
// when it was taken before. An exception of the source ends the reader and is rethrown by every take from then on
// (at the latest by the one waiting on that frame); the destructor stops the reader and joins it, also while it
// waits on the window. Host code only.
#pragma once
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <exception>
#include <functional>
#include <map>
#include <mutex>
#include <thread>
#include <vector>

namespace sart {

class FrameReadahead {
   public:
    using Source = std::function<std::vector<double>(int64_t)>;  // series index -> the frame (never empty)
    FrameReadahead(int64_t nframes, int64_t ahead, Source source)
        : nframes_(nframes), ahead_(ahead), source_(std::move(source)), reader_([this] { run(); }) {}
    ~FrameReadahead() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        if (reader_.joinable()) reader_.join();
    }
    FrameReadahead(const FrameReadahead&) = delete;
    FrameReadahead& operator=(const FrameReadahead&) = delete;

    std::vector<double> take(int64_t k) {
        std::vector<double> f;
        {
            std::unique_lock<std::mutex> lk(mu_);
            cv_.wait(lk, [&] { return err_ || ready_.count(k) || k < reader_next_; });
            if (err_) std::rethrow_exception(err_);
            auto it = ready_.find(k);
            if (it != ready_.end()) {
                f = std::move(it->second);
                ready_.erase(it);
            }
            consumed_ = std::max(consumed_, k + 1);
            cv_.notify_all();
        }
        if (f.empty()) {  // asked again (a re-solve after a device all-reduce failure): read it here
            std::lock_guard<std::mutex> io(io_mu_);
            f = source_(k);
        }
        return f;
    }
    double reader_ms() const {  // the reader thread's time in the source
        std::lock_guard<std::mutex> lk(mu_);
        return reader_ms_;
    }

   private:
    void run() {
        try {
            for (int64_t k = 0; k < nframes_; ++k) {
                {
                    std::unique_lock<std::mutex> lk(mu_);
                    cv_.wait(lk, [&] { return stop_ || k < consumed_ + ahead_; });
                    if (stop_) return;
                }
                std::vector<double> f;
                const auto tr = std::chrono::steady_clock::now();
                {
                    std::lock_guard<std::mutex> io(io_mu_);
                    f = source_(k);
                }
                const double rms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tr).count();
                std::lock_guard<std::mutex> lk(mu_);
                reader_ms_ += rms;
                ready_.emplace(k, std::move(f));
                reader_next_ = k + 1;
                cv_.notify_all();
            }
        } catch (...) {
            std::lock_guard<std::mutex> lk(mu_);
            err_ = std::current_exception();
            stop_ = true;
            cv_.notify_all();
        }
    }

    const int64_t nframes_, ahead_;
    const Source source_;
    mutable std::mutex mu_;
    std::mutex io_mu_;  // one source call at a time (the reader's and a re-read's)
    std::condition_variable cv_;
    std::map<int64_t, std::vector<double>> ready_;  // frames read ahead, by series index
    int64_t consumed_ = 0, reader_next_ = 0;
    double reader_ms_ = 0.0;
    bool stop_ = false;
    std::exception_ptr err_;
    std::thread reader_;  // last: it starts with every other member built
};

}  // namespace sart
