// line_find_check.cpp -- csrc/hostlogic/line_find.hpp (gr4pm_find_line) as a stand-alone program for
// -fsanitize=undefined,address: spectra in heap blocks of exactly n bins, windows that wrap, flat spectra, spectra with
// zeros, the minimum n_bins = 2 guard_bins + 3, n_bins = n, a line whose neighbour lies outside the window, and an exact
// Gaussian line, whose logarithm is the parabola the interpolation assumes.
#include <cmath>
#include <cstdio>
#include <memory>

#include "hostlogic/line_find.hpp"

using namespace gr4pm::hostlogic;

static int g_cases = 0, g_failures = 0;

static void expect(bool ok, const char* name)
{
    ++g_cases;
    if (!ok) {
        ++g_failures;
        std::printf("FAIL %s\n", name);
    }
}

static std::unique_ptr<double[]> make(size_t n, double v)
{
    std::unique_ptr<double[]> p(new double[n]);
    for (size_t i = 0; i < n; ++i) p[i] = v;
    return p;
}

int main()
{
    const size_t n = 64;
    {
        auto p = make(n, 1.0); // flat: the first bin of the window, no margin, no interpolation
        const Line l = find_line(p.get(), n, 60, 10, 2);
        expect(l.bin == 60 && l.found == 1 && l.margin_db == 0.0 && l.snr_db == 0.0 && l.frequency == 60.0 / 64.0 - 1.0, "flat, wrapping");
    }
    {
        auto p = make(n, 0.0); // all zero: nothing found
        const Line l = find_line(p.get(), n, 0, n, 2);
        expect(l.found == 0 && l.snr_db == 0.0 && l.margin_db == 0.0 && l.frequency == 0.0 && l.bin == 0, "zeros");
    }
    {
        auto p = make(n, 0.0); // one bin above zeros: infinite ratios, no interpolation
        p[63] = 3.0;
        const Line l = find_line(p.get(), n, 62, 7, 2);
        expect(l.found == 1 && l.bin == 63 && std::isinf(l.snr_db) && std::isinf(l.margin_db) && l.frequency == -1.0 / 64.0, "one bin above zeros");
    }
    {
        auto p = make(n, 1.0); // the peak's neighbour 0 lies outside the window [1, 8) and is used all the same
        p[1] = 8.0, p[0] = 4.0, p[2] = 2.0;
        const Line l = find_line(p.get(), n, 1, 7, 2);
        const double la = std::log(4.0), lb = std::log(8.0), lc = std::log(2.0);
        const double d = 0.5 * (la - lc) / (la - 2.0 * lb + lc);
        expect(l.bin == 1 && std::fabs(l.frequency - (1.0 + d) / 64.0) < 1e-15 && d < 0.0, "a neighbour outside the window");
        expect(std::fabs(l.margin_db - 10.0 * std::log10(8.0)) < 1e-12 && l.floor == 1.0, "margin skips the guard bins");
    }
    {
        auto p = make(n, 1.0); // the minimum window with no guard: three bins; the first maximum of two equal ones
        p[10] = 5.0, p[11] = 5.0;
        const Line l = find_line(p.get(), n, 9, 3, 0);
        expect(l.bin == 10 && l.floor == 5.0 && l.margin_db == 0.0 && l.snr_db == 0.0, "three bins, two equal maxima");
        expect(!line_window_valid(n, 9, 2, 0) && !line_window_valid(n, 9, 6, 2) && line_window_valid(n, 9, 7, 2) &&
                   !line_window_valid(n, 64, 7, 2) && !line_window_valid(n, 0, 65, 2) && line_window_valid(n, 63, 64, 2) &&
                   !line_window_valid(0, 0, 0, 0) && !line_window_valid(n, 0, 64, UINT64_MAX / 2),
               "window validity");
    }
    {
        auto p = make(n, 0.0); // a convex triple (curvature >= 0) and a zero neighbour: no interpolation
        p[20] = 4.0, p[19] = 4.0, p[21] = 4.0;
        expect(find_line(p.get(), n, 0, n, 2).frequency == 19.0 / 64.0, "flat top: the first maximum, no shift");
        p[19] = 0.0;
        expect(find_line(p.get(), n, 0, n, 2).frequency == 20.0 / 64.0, "zero neighbour: no shift");
    }
    for (int i = 0; i < 40; ++i) { // exact Gaussian lines anywhere on the circle, across bin 0 too
        const double centre = 0.37 + 1.6 * i;
        auto p = make(n, 0.0);
        for (size_t k = 0; k < n; ++k) {
            double dist = std::fabs(static_cast<double>(k) - centre);
            dist = dist < 64.0 - dist ? dist : 64.0 - dist;
            p[k] = std::exp(-0.5 * dist * dist) + 1e-30;
        }
        const Line l = find_line(p.get(), n, (static_cast<size_t>(centre) + n - 5) % n, 11, 2);
        double want = centre / 64.0;
        want -= std::floor(want + 0.5);
        expect(std::fabs(l.frequency - want) < 1e-9 && l.frequency >= -0.5 && l.frequency < 0.5, "Gaussian line");
    }
    {
        auto p = make(2048, 1.0); // clamp: a neighbour almost as high as the peak
        p[100] = 2.0, p[101] = 2.0 - 1e-15, p[99] = 1e-300;
        const Line l = find_line(p.get(), 2048, 0, 2048, 2);
        expect(l.bin == 100 && l.frequency <= 100.5 / 2048.0 && l.frequency > 100.0 / 2048.0, "clamped to half a bin");
    }
    std::printf("line_find_check: %d cases, %d failures\n", g_cases, g_failures);
    return g_failures ? 1 : 0;
}
