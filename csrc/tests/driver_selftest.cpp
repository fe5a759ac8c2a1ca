// Stand-alone self-test of the native driver's host-only units (built with sanitizers by
// tests/test_driver_sanitizers.py): the bounded frame read-ahead (csrc/driver/frame_readahead.hpp) on a synthetic
// source, the --profile JSON-line builder (csrc/driver/profile_lines.hpp) against the operator<< chains it replaced, and
// the series runs' order rules (csrc/driver/series_order.hpp).
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <sstream>
#include <stdexcept>

#include "../driver/frame_readahead.hpp"
#include "../driver/profile_lines.hpp"
#include "../driver/series_order.hpp"

using namespace sart;

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                              \
        }                                                              \
    } while (0)

namespace {

std::vector<double> frame_of(int64_t k) { return {(double)k, 2.0 * k + 1.0, -0.5 * k}; }

// A source that counts its calls per frame, checks the window against the newest frame asked for (set before every
// take, so consumed <= asked at any time) and lets the test wait until a given frame has been read.
struct Source {
    int64_t ahead;
    int64_t fail_at = -1;
    std::atomic<int64_t> asked{0};
    std::atomic<bool> window_broken{false};
    std::mutex mu;
    std::condition_variable cv;
    std::map<int64_t, int> calls;
    std::vector<double> operator()(int64_t k) {
        if (k >= asked.load() + ahead) window_broken = true;
        {
            std::lock_guard<std::mutex> lk(mu);
            ++calls[k];
        }
        cv.notify_all();
        if (k == fail_at) throw std::runtime_error("synthetic read error");
        return frame_of(k);
    }
    void wait_for(int64_t k) {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return calls.count(k) > 0; });
    }
    int count(int64_t k) {
        std::lock_guard<std::mutex> lk(mu);
        return calls.count(k) ? calls[k] : 0;
    }
};

std::vector<double> take(FrameReadahead& ra, Source& s, int64_t k) {
    int64_t a = s.asked.load();
    while (a < k + 1 && !s.asked.compare_exchange_weak(a, k + 1)) {
    }
    return ra.take(k);
}

void test_readahead() {
    {  // in order, through a window narrower than the series
        Source s{3};
        FrameReadahead ra(20, 3, [&](int64_t k) { return s(k); });
        s.wait_for(2);  // the reader fills the window before anything is taken, and stops there
        CHECK(s.count(3) == 0);
        for (int64_t k = 0; k < 20; ++k) CHECK(take(ra, s, k) == frame_of(k));
        CHECK(!s.window_broken);
        for (int64_t k = 0; k < 20; ++k) CHECK(s.count(k) == 1);
        CHECK(ra.reader_ms() >= 0.0);
    }
    {  // out of order, and a frame taken twice is read again through the source
        Source s{4};
        FrameReadahead ra(8, 4, [&](int64_t k) { return s(k); });
        CHECK(take(ra, s, 2) == frame_of(2));
        CHECK(take(ra, s, 0) == frame_of(0));
        CHECK(take(ra, s, 1) == frame_of(1));
        CHECK(take(ra, s, 5) == frame_of(5));
        CHECK(take(ra, s, 3) == frame_of(3));
        CHECK(s.count(0) == 1);
        CHECK(take(ra, s, 0) == frame_of(0));
        CHECK(s.count(0) == 2);
        CHECK(take(ra, s, 4) == frame_of(4));
        CHECK(take(ra, s, 7) == frame_of(7));
        CHECK(take(ra, s, 6) == frame_of(6));
        CHECK(!s.window_broken);
    }
    // The source's exception on frame 5. A stored error is rethrown by the next take of any frame (the batch cannot
    // go on without frame 5), so it may surface from any take made after frame 5 entered the window, and must surface
    // from the take that waits on frame 5.
    auto throws = [](FrameReadahead& ra, Source& s, int64_t k) {
        try {
            CHECK(take(ra, s, k) == frame_of(k));
        } catch (const std::runtime_error& e) {
            CHECK(std::string(e.what()) == "synthetic read error");
            return true;
        }
        return false;
    };
    {  // window 1: frame 5 is read only once frame 4 has been taken, so takes 0 .. 4 succeed and take 5 throws
        Source s{1};
        s.fail_at = 5;
        FrameReadahead ra(10, 1, [&](int64_t k) { return s(k); });
        for (int64_t k = 0; k < 5; ++k) CHECK(!throws(ra, s, k));
        CHECK(throws(ra, s, 5));
        CHECK(s.count(6) == 0);  // the reader stopped at the error
    }
    {  // window 4: frame 5 enters the window with take 1 (consumed = 2), so take 0 and take 1 succeed; a later take
       // may throw, take 5 does at the latest
        Source s{4};
        s.fail_at = 5;
        FrameReadahead ra(10, 4, [&](int64_t k) { return s(k); });
        CHECK(!throws(ra, s, 0));
        CHECK(!throws(ra, s, 1));
        bool thrown = false;
        for (int64_t k = 2; k <= 5 && !thrown; ++k) thrown = throws(ra, s, k);
        CHECK(thrown);
    }
    {  // destroyed while the reader waits on the window (nothing taken): the destructor stops and joins it
        Source s{2};
        FrameReadahead ra(100, 2, [&](int64_t k) { return s(k); });
        s.wait_for(1);
    }
    {  // an empty series
        Source s{2};
        FrameReadahead ra(0, 2, [&](int64_t k) { return s(k); });
    }
}

void test_json_line() {
    const double dv[] = {0.0, 1.0 / 3.0, 1e-7, 123456789.0, 2.5e10, -17.25, 1048576.0, 0.1 + 0.2, 6.02214076e23};
    const std::string path = "multi-frame \"f16\" \\ split";
    std::ostringstream a, b;
    {
        JsonLine j(a);
        j("load", true)("off", false)("i", -3)("i64", (int64_t)-1234567890123)("u64", (uint64_t)18446744073709551615ull)(
            "size", (size_t)42)("zero_or_one", true ? 1 : 0);
        for (double v : dv) j("d", v);
        j.open("rank0")("load_s", 0.125)("blocks", (uint64_t)7);
        j.close()("solver_path", path)("storage", "fp32")("c_str", path.c_str())("driver", "native").end();
    }
    b << "{\"load\": true, \"off\": " << (false ? "true" : "false") << ", \"i\": " << -3 << ", \"i64\": "
      << (int64_t)-1234567890123 << ", \"u64\": " << (uint64_t)18446744073709551615ull << ", \"size\": " << (size_t)42
      << ", \"zero_or_one\": " << 1;
    for (double v : dv) b << ", \"d\": " << v;
    b << ", \"rank0\": {\"load_s\": " << 0.125 << ", \"blocks\": " << (uint64_t)7 << "}"
      << ", \"solver_path\": \"" << json_escape(path) << "\", \"storage\": \"fp32\", \"c_str\": \"" << json_escape(path)
      << "\", \"driver\": \"" << json_escape("native") << "\"}\n";
    CHECK(a.str() == b.str());
    CHECK(json_escape(path) == "multi-frame \\\"f16\\\" \\\\ split");
    std::ostringstream e;
    JsonLine(e).end();
    CHECK(e.str() == "{}\n");
}

void test_in_order() {
    using Emitted = std::vector<int64_t>;
    {  // first index 0, a move-only payload: puts 2, 0, 1, 4, 3 emit nothing; 0; 1, 2; nothing; 3, 4
        InOrder<std::unique_ptr<int64_t>> q;
        Emitted out;
        auto emit = [&](int64_t k, std::unique_ptr<int64_t>&& item) {
            const std::unique_ptr<int64_t> mine = std::move(item);  // moved out, not copied
            CHECK(mine && *mine == 10 * k);
            out.push_back(k);
        };
        q.drain(emit);  // nothing put yet
        CHECK(out.empty() && q.empty());
        const int64_t puts[] = {2, 0, 1, 4, 3};
        const Emitted after[] = {{}, {0}, {0, 1, 2}, {0, 1, 2}, {0, 1, 2, 3, 4}};
        for (int i = 0; i < 5; ++i) {
            q.put(puts[i], std::make_unique<int64_t>(10 * puts[i]));
            q.drain(emit);
            CHECK(out == after[i]);
            q.drain(emit);  // nothing ready: nothing more
            CHECK(out == after[i]);
            CHECK(q.empty() == (i == 2 || i == 4));
        }
    }
    {  // first index 1 (the lead frame was written before the series): an item at 0 never leaves, 1 leaves at once
        InOrder<int> q(1);
        Emitted out;
        auto emit = [&](int64_t k, int&& item) {
            CHECK(item == (int)k + 100);
            out.push_back(k);
        };
        q.put(0, 100);
        q.drain(emit);
        CHECK(out.empty() && !q.empty());
        q.put(1, 101);
        q.drain(emit);
        CHECK(out == Emitted{1});
        q.put(3, 103), q.put(2, 102);
        q.drain(emit);
        CHECK((out == Emitted{1, 2, 3}));
        CHECK(!q.empty());  // (item 0 alone)
    }
}

void test_column_count() {
    {  // one column per frame: every arrival completes its frame
        ColumnCount c(4, 1);
        for (int64_t j : {2, 0, 3, 1}) {
            CHECK(c.frame(j) == j && c.column(j) == 0);
            CHECK(c.arrived(j));
        }
    }
    {  // nc = 3, T = 2, arrivals interleaved across the frames: frame 1 completes at 5, frame 0 at 2, each once
        ColumnCount c(2, 3);
        std::vector<int64_t> completed;
        for (int64_t j : {3, 0, 4, 1, 5, 2})
            if (c.arrived(j)) completed.push_back(j);
        CHECK((completed == std::vector<int64_t>{5, 2}));
        CHECK(c.frame(5) == 1 && c.column(5) == 2 && c.frame(2) == 0 && c.column(2) == 2);
    }
    {  // T nc = 2^31 + 2: the last virtual index in 64-bit arithmetic
        const int64_t nc = ((int64_t)1 << 30) + 1, T = 2, last = T * nc - 1;
        CHECK(last == ((int64_t)1 << 31) + 1);
        ColumnCount c(T, nc);
        CHECK(c.frame(last) == 1 && c.column(last) == nc - 1);
        CHECK(c.frame(nc) == 1 && c.column(nc) == 0 && c.frame(nc - 1) == 0 && c.column(nc - 1) == nc - 1);
        CHECK(!c.arrived(last));
    }
}

}  // namespace

int main() {
    test_readahead();
    test_json_line();
    test_in_order();
    test_column_count();
    std::cout << "driver selftest OK" << std::endl;
    return 0;
}
