// Self-test of the fit diagnostics' host code (csrc/native/fit.cpp), built with AddressSanitizer +
// UndefinedBehaviorSanitizer and run as a plain executable (tests/test_fit_sanitizers.py): cpu_fit_forward on dense
// rows and on CSR rows against a long-double reference, fit_statistics on hand cases, and FitWriter on a solution
// file written by SolutionWriter -- create the /fit group, write its rows, replace an existing group, read back.
// Exit code 0 = all checks passed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "../native/fit.hpp"
#include "../native/frames.hpp"
#include "../native/h5.hpp"
#include "../native/sparse_csr.hpp"

using namespace sart;

static int failures = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                         \
        }                                                                       \
    } while (0)

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : "/tmp";
    std::mt19937 rng(11);
    std::uniform_real_distribution<float> U(0.f, 1.f);
    std::normal_distribution<double> N(0.0, 1.0);

    // dense rows with padding columns and a padded X: neither padding is read
    const int64_t P = 37, V = 101, ld = 128, ldx = 104, nv = 5;
    std::vector<float> A(P * ld, 3.f);
    for (int64_t p = 0; p < P; ++p)
        for (int64_t v = 0; v < V; ++v) A[p * ld + v] = U(rng) < 0.3f ? 0.f : U(rng);
    std::vector<double> X(nv * ldx, std::nan(""));
    for (int j = 0; j < nv; ++j)
        for (int64_t v = 0; v < V; ++v) X[j * ldx + v] = N(rng);
    std::vector<double> F(nv * P, -1.0);
    cpu_fit_forward(A.data(), P, V, ld, X.data(), ldx, (int)nv, F.data(), P);
    for (int j = 0; j < nv; ++j)
        for (int64_t p = 0; p < P; ++p) {
            long double s = 0, m = 0;
            for (int64_t v = 0; v < V; ++v) {
                s += (long double)A[p * ld + v] * X[j * ldx + v];
                m += std::fabs((long double)A[p * ld + v] * X[j * ldx + v]);
            }
            CHECK(std::fabs((double)(F[j * P + p] - s)) <= 2.0 * (V + 2) * std::ldexp(1.0, -53) * (double)m);
        }
    // one vector alone gives the same bits as inside the group
    std::vector<double> F1(P);
    cpu_fit_forward(A.data(), P, V, ld, X.data() + 3 * ldx, ldx, 1, F1.data(), P);
    for (int64_t p = 0; p < P; ++p) CHECK(F1[p] == F[3 * P + p]);

    // CSR rows of the same matrix (an empty row among them)
    std::vector<int64_t> er;
    std::vector<int32_t> ec;
    std::vector<float> ev;
    for (int64_t p = 0; p < P; ++p)
        for (int64_t v = 0; v < V; ++v)
            if (p != 4 && A[p * ld + v] != 0.f) er.push_back(p), ec.push_back((int32_t)v), ev.push_back(A[p * ld + v]);
    const HostCsr rows = csr_from_entries(P, V, er, ec, ev);
    std::vector<double> Fs(nv * P, -1.0);
    cpu_fit_forward(rows, X.data(), ldx, (int)nv, Fs.data(), P);
    for (int j = 0; j < nv; ++j)
        for (int64_t p = 0; p < P; ++p)
            CHECK(p == 4 ? Fs[j * P + p] == 0.0
                         : std::fabs(Fs[j * P + p] - F[j * P + p]) <= 1e-12 * (1.0 + std::fabs(F[j * P + p])));
    bool threw = false;
    try {
        cpu_fit_forward(rows, X.data(), V - 1, 1, Fs.data(), P);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    CHECK(threw);

    // statistics: saturated pixels, a camera without a valid pixel, a ray length at the threshold
    {
        const std::vector<double> g = {1.0, 2.0, -1.0, -1.0, 3.0, 1.0};
        const std::vector<double> f = {0.5, 2.0, 9.0, 9.0, 1.0, 0.0};
        const std::vector<double> ell = {1.0, 1.0, 1.0, 1.0, 1.0, 0.25};
        const FitStats s = fit_statistics(f.data(), g.data(), ell.data(), 6, 0.25, {2, 2, 2});
        CHECK(s.pixels == 3 && s.pixels_camera == (std::vector<int64_t>{2, 0, 1}));
        CHECK(s.residual_norm == std::sqrt(0.25 + 4.0) && s.residual_max == 2.0);
        CHECK(s.measurement_norm == std::sqrt(1.0 + 4.0 + 9.0));
        CHECK(s.residual_norm_camera[1] == 0.0 && s.measurement_norm_camera[2] == 3.0);
        const std::vector<double> neg(6, -1.0);
        const FitStats z = fit_statistics(f.data(), neg.data(), ell.data(), 6, 0.25, {6});
        CHECK(z.pixels == 0 && z.residual_norm == 0.0 && z.measurement_norm == 0.0 && z.residual_max == 0.0);
        threw = false;
        try {
            fit_statistics(f.data(), g.data(), ell.data(), 6, 0.25, {2, 2});
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        CHECK(threw);
    }

    // FitWriter on a solution file: create, write, replace
    {
        const std::string path = dir + "/fit_selftest.h5";
        const uint64_t nvox = 7, npix = 9, T = 3;
        {
            SolutionWriter w(path, {"cam_a", "cam_b"}, nvox, 2);
            for (uint64_t k = 0; k < T; ++k)
                w.add(std::vector<double>(nvox, 1.0 + (double)k), 0, 0.1 * (double)k, {0.1 * (double)k, 0.1 * (double)k}, 5);
            w.flush();
        }
        const std::vector<double> t = read_solution_times(path);
        CHECK(t.size() == T && t[2] == 0.1 * 2.0);
        const std::vector<double> x = read_solution_rows(path, 1, 2, nvox);
        CHECK(x.size() == 2 * nvox && x[0] == 2.0 && x[nvox] == 3.0);
        CHECK(read_solution_times(dir + "/no_such_file.h5").empty());
        threw = false;
        try {
            read_solution_rows(path, 2, 2, nvox);
        } catch (const Error&) {
            threw = true;
        }
        CHECK(threw);
        for (int round = 0; round < 2; ++round) {  // the second round replaces the first round's group
            FitWriter fw(path, T, npix, 2);
            for (uint64_t k = 0; k < T; ++k) {
                std::vector<double> img(npix);
                for (uint64_t p = 0; p < npix; ++p) img[p] = 100.0 * round + 10.0 * (double)k + (double)p;
                FitStats s;
                s.residual_norm = 1.0 + (double)k + round;
                s.measurement_norm = 2.0;
                s.residual_max = 0.5;
                s.pixels = 8;
                s.residual_norm_camera = {0.25, 0.75};
                s.measurement_norm_camera = {1.0, 1.5};
                s.pixels_camera = {3, 5};
                fw.write(k, img.data(), s);
            }
            threw = false;
            try {
                fw.write(T, nullptr, FitStats{});
            } catch (const Error&) {
                threw = true;
            }
            CHECK(threw);
            SART_H5_LOCK;
            H5Id f = h5_open_file(path);
            const std::vector<double> img = h5_read_f64(f, "fit/image");
            CHECK(img.size() == T * npix && img[npix + 2] == 100.0 * round + 12.0);
            const std::vector<double> rn = h5_read_f64(f, "fit/residual_norm");
            CHECK(rn.size() == T && rn[2] == 3.0 + round);
            const std::vector<int64_t> pc = h5_read_i64(f, "fit/pixels_camera");
            CHECK(pc.size() == 2 * T && pc[0] == 3 && pc[5] == 5);
            const std::vector<int64_t> px = h5_read_i64(f, "fit/pixels");
            CHECK(px.size() == T && px[1] == 8);
            H5Id d = h5_open_dataset(f, "fit/image");
            CHECK(h5_dims(d) == (std::vector<hsize_t>{T, npix}));
            // the solution is untouched
            CHECK(h5_read_f64(f, "solution/value").size() == T * nvox);
        }
    }

    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("fit selftest OK\n");
    return 0;
}
