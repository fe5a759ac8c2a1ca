// Self-test of the beta scan's host code (csrc/native/lcurve.cpp), built with AddressSanitizer +
// UndefinedBehaviorSanitizer by tests/test_lcurve_sanitizers.py: lcurve_corner on hand cases (a right angle, an
// invalid point bridged, everything invalid, a fallback out of the valid points), and ScanWriter next to the
// solution writer on one file -- columns written out of order, read back across frame borders, the frame rows, and
// /solution added to the file the scan created.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../native/frames.hpp"
#include "../native/lcurve.hpp"

using namespace sart;

namespace {
int failures = 0;
void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        ++failures;
    }
}
}  // namespace

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : ".";
    {  // down, then right: one corner with cross > 0
        const double rho[3] = {1, 1, 2}, eta[3] = {4, 1, 1};
        const uint8_t ok[3] = {1, 1, 1};
        const LcurveCorner c = lcurve_corner(rho, eta, ok, 3, 0);
        expect(c.found == 1 && c.selected == 1 && c.curvature[1] > 0, "right angle");
        expect(std::isnan(c.curvature[0]) && std::isnan(c.curvature[2]), "end points have no curvature");
    }
    {  // the invalid point in the middle is bridged: the same curvature as without it
        const double rho[4] = {1, 1, 7, 2}, eta[4] = {4, 1, NAN, 1};
        const uint8_t ok[4] = {1, 1, 1, 1};
        const LcurveCorner c = lcurve_corner(rho, eta, ok, 4, 0);
        const double rho3[3] = {1, 1, 2}, eta3[3] = {4, 1, 1};
        const LcurveCorner c3 = lcurve_corner(rho3, eta3, ok, 3, 0);
        expect(c.selected == 1 && std::isnan(c.curvature[2]) && c.curvature[1] == c3.curvature[1], "bridged point");
    }
    {  // nothing valid: the fallback as given; no points at all
        const double rho[3] = {1, 2, 3}, eta[3] = {3, 2, 1};
        const uint8_t ok[3] = {0, 0, 0};
        const LcurveCorner c = lcurve_corner(rho, eta, ok, 3, 2);
        expect(c.found == 0 && c.selected == 2 && c.curvature.size() == 3, "all invalid");
        const LcurveCorner e = lcurve_corner(rho, eta, ok, 0, 0);
        expect(e.found == 0 && e.curvature.empty(), "no points");
    }
    {  // a horizontal line has no corner; the fallback moves to the nearest valid point, ties to the smaller index
        const double rho[5] = {1, 2, 4, 8, 16}, eta[5] = {3, 3, 3, 3, 3};
        const uint8_t ok[5] = {1, 1, 0, 1, 1};
        expect(lcurve_corner(rho, eta, ok, 5, 2).selected == 1, "fallback tie");
        expect(lcurve_corner(rho, eta, ok, 5, 4).selected == 4, "valid fallback");
    }
    {
        const uint64_t T = 3, nb = 4, nv = 10;
        const double beta[4] = {0, 1, 2, 3};
        const std::string fn = dir + "/lcurve_selftest.h5";
        SolutionWriter w(fn, {"cam_a"}, nv, 2, false, true);  // a cache of 2: a background write during the pass
        ScanWriter s(fn, T, nb, nv, beta);
        std::vector<double> x(nv);
        for (uint64_t j = 0; j < T * nb; ++j) {
            const uint64_t jj = (j * 5) % (T * nb);  // out of order
            for (uint64_t v = 0; v < nv; ++v) x[v] = (double)(jj * 100 + v);
            s.write_column(jj / nb, jj % nb, x.data(), (int32_t)(jj % 2) - 1, (int32_t)jj);
        }
        s.close();
        std::vector<double> X(5 * nv);
        s.read_columns(3, 5, X.data());  // across the border of frames 0 and 1
        bool same = true;
        for (uint64_t r = 0; r < 5; ++r)
            for (uint64_t v = 0; v < nv; ++v) same = same && X[r * nv + v] == (double)((3 + r) * 100 + v);
        expect(same, "columns read back");
        for (uint64_t k = 0; k < T; ++k) {
            const double rho[4] = {1, 2, 3, 4}, eta[4] = {4, 3, 2, 1}, curv[4] = {NAN, 0.5, -1, NAN};
            s.write_frame(k, rho, eta, curv, 1, 1);
            s.read_columns(k * nb + 1, 1, x.data());
            s.close();
            w.add(x, 0, 0.1 * (double)k, {0.1 * (double)k}, 7);
        }
        w.flush();
        const StoredSolutions st = read_solution_file(fn);
        expect(st.time.size() == T && st.last_solution.size() == nv && st.last_solution[1] == 901.0,
               "/solution added to the scan's file");
        bool threw = false;
        try {
            s.write_column(T, 0, x.data(), 0, 0);
        } catch (const Error&) {
            threw = true;
        }
        expect(threw, "a column out of bounds is refused");
    }
    if (failures) return 1;
    std::printf("lcurve selftest OK\n");
    return 0;
}
