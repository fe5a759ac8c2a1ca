// Stand-alone self-test of the native driver's host-only units (built with sanitizers by
// tests/test_driver_sanitizers.py): the bounded frame read-ahead (csrc/driver/frame_readahead.hpp) on a synthetic
// source, and the --profile JSON-line builder (csrc/driver/profile_lines.hpp) against the operator<< chains it replaced.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <stdexcept>

#include "../driver/frame_readahead.hpp"
#include "../driver/profile_lines.hpp"

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

}  // namespace

int main() {
    test_readahead();
    test_json_line();
    std::cout << "driver selftest OK" << std::endl;
    return 0;
}
