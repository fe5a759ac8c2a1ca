// Self-test of the phantom study's host code (csrc/native/phantom.cpp), built with AddressSanitizer +
// UndefinedBehaviorSanitizer by tests/test_phantom_sanitizers.py: the scores on hand-made sums (zero denominators
// included), the phantom file's reader on fp32 and fp64 files with and without times and on every file it must refuse,
// and PhantomWriter next to the solution writer on one file.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../native/frames.hpp"
#include "../native/phantom.hpp"

using namespace sart;

namespace {
int failures = 0;
void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        ++failures;
    }
}
// the reader refuses `fn` with a message that names `dataset`
void refused(const std::string& fn, uint64_t nvoxel, const char* dataset, const char* what) {
    bool ok = false;
    try {
        PhantomFile f(fn, nvoxel);
    } catch (const Error& e) {
        ok = std::string(e.what()).find(dataset) != std::string::npos;
    }
    expect(ok, what);
}
}  // namespace

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : ".";
    {  // s_t s_x s_tt s_xx s_xt s_dd s_in m_d m_t m_x
        const double s[kPhantomSumCount] = {4, 3, 8, 2, 3, 4, 2.5, 1.5, 2, 1};
        const PhantomScores r = phantom_scores(s);
        expect(r.rel_l2 == std::sqrt(4.0 / 8.0) && r.cosine == 3.0 / std::sqrt(2.0 * 8.0), "rel_l2 and cosine");
        expect(r.total_ratio == 0.75 && r.peak_ratio == 0.5 && r.max_error == 0.75, "ratios");
        expect(r.inside_fraction == 2.5 / 3.0, "inside fraction");
        const double dark[kPhantomSumCount] = {0, 3, 0, 2, 0, 2, 0, 1, 0, 1};  // the all-zero truth
        const PhantomScores z = phantom_scores(dark);
        expect(std::isnan(z.rel_l2) && std::isnan(z.cosine) && std::isnan(z.total_ratio) && std::isnan(z.peak_ratio) &&
                   std::isnan(z.max_error) && z.inside_fraction == 0.0, "zero denominators give NaN");
        const double none[kPhantomSumCount] = {1, 0, 1, 0, 0, 1, 0, 1, 1, 0};  // the all-zero column
        const PhantomScores e = phantom_scores(none);
        expect(e.rel_l2 == 1.0 && std::isnan(e.cosine) && std::isnan(e.inside_fraction) && e.total_ratio == 0.0,
               "an empty column");
    }
    const uint64_t n = 3, nv = 5;
    std::vector<double> value(n * nv);
    for (uint64_t i = 0; i < n * nv; ++i) value[i] = 0.25 * (double)(i % 7);
    {
        const std::string fn = dir + "/phantom_selftest_in.h5";
        write_phantom_file(fn, value.data(), n, nv, nullptr, false);
        PhantomFile f(fn, nv);
        expect(f.count() == n && f.times().size() == n && f.times()[2] == 2.0, "default times");
        std::vector<double> rows(2 * nv);
        f.read_rows(1, 2, rows.data());
        bool same = true;
        for (uint64_t i = 0; i < 2 * nv; ++i) same = same && rows[i] == value[nv + i];
        expect(same, "fp64 rows read back");
        const double t[3] = {0.5, 0.75, 4.0};
        write_phantom_file(fn, value.data(), n, nv, t, true);
        PhantomFile g(fn, nv);
        g.read_rows(0, 1, rows.data());
        expect(g.times()[1] == 0.75 && rows[3] == 0.75, "fp32 values and given times");
        bool threw = false;
        try {
            g.read_rows(2, 2, rows.data());
        } catch (const Error&) {
            threw = true;
        }
        expect(threw, "rows beyond the file are refused");
        refused(fn, nv + 1, "phantom/value", "wrong voxel count");
        write_phantom_file(fn, value.data(), 0, nv, nullptr, false);
        refused(fn, nv, "phantom/value", "n = 0");
        std::vector<double> bad = value;
        bad[7] = -1e-300;
        write_phantom_file(fn, bad.data(), n, nv, nullptr, false);
        refused(fn, nv, "phantom/value", "negative entry");
        bad[7] = INFINITY;
        write_phantom_file(fn, bad.data(), n, nv, nullptr, false);
        refused(fn, nv, "phantom/value", "infinite entry");
        bad[7] = NAN;
        write_phantom_file(fn, bad.data(), n, nv, nullptr, true);
        refused(fn, nv, "phantom/value", "NaN entry");
        const double flat[3] = {0.0, 1.0, 1.0};
        write_phantom_file(fn, value.data(), n, nv, flat, false);
        refused(fn, nv, "phantom/time", "times that do not increase");
        write_phantom_file(fn, value.data(), n, nv, t, false);
        {  // two times for three phantoms
            SART_H5_LOCK;
            H5Id f2 = h5_open_file(fn, true);
            H5Ldelete(f2, "phantom/time", H5P_DEFAULT);
            h5_write_f64(f2, "phantom/time", {2}, t);
        }
        refused(fn, nv, "phantom/time", "a time missing");
        {
            SART_H5_LOCK;
            H5Id f2 = h5_create_file(fn);
            H5Id grp = h5_create_group(f2, "phantom");
        }
        refused(fn, nv, "phantom/value", "missing dataset");
    }
    {
        const uint64_t nc = 3, npix = 4;
        const std::string fn = dir + "/phantom_selftest_out.h5";
        const double t[3] = {0.0, 1.0, 2.0};
        SolutionWriter w(fn, {"cam_a"}, nv, 2, false, true);
        PhantomWriter p(fn, n, nc, npix, "truth.h5", t, false);
        std::vector<double> sums(nc * kPhantomSumCount), x(nv, 1.0), image(n * npix, 2.0);
        const int32_t status[3] = {0, -1, 0}, iters[3] = {5, 6, 7};
        for (uint64_t k = 0; k < n; ++k) {
            const uint64_t kk = (k * 2) % n;  // out of order
            for (size_t i = 0; i < sums.size(); ++i) sums[i] = (double)(kk + i % 4);
            p.write_phantom(kk, sums.data(), status, iters);
            w.add(x, 0, t[k], {t[k]}, 7);
        }
        p.write_images(image.data());
        w.flush();
        const StoredSolutions st = read_solution_file(fn);
        expect(st.time.size() == n, "/solution added to the phantom's file");
        SART_H5_LOCK;
        H5Id f = h5_open_file(fn);
        expect(h5_read_f64(f, "phantom/sums").size() == n * nc * kPhantomSumCount, "sums");
        expect(h5_read_f64(f, "phantom/image")[5] == 2.0 && h5_read_i32(f, "phantom/iterations")[4] == 6, "rows");
        expect(h5_attr_string(f, "phantom", "file") == "truth.h5", "the phantom file's name");
        for (const char* name : kPhantomScoreNames)
            expect(h5_read_f64(f, std::string("phantom/") + name).size() == n * nc, name);
        bool threw = false;
        try {
            p.write_phantom(n, sums.data(), status, iters);
        } catch (const Error&) {
            threw = true;
        }
        expect(threw, "a phantom out of bounds is refused");
    }
    if (failures) return 1;
    std::printf("phantom selftest OK\n");
    return 0;
}
