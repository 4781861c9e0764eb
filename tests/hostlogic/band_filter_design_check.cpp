// Checks csrc/hostlogic/band_filter_design.hpp (the designer behind gr4pm_band_filter_taps) against a
// double transform of its taps on 2^16 frequencies: at every frequency at least half a transition width
// (A - 7.95) / (14.36 (L - 1)) from every merged band edge, |H(f) e^{2 pi j f c} - ideal(f)| <= 2 n_bands 10^(-A / 20), in both
// modes, for four designs; the merging of overlapping, touching and wrapping bands; stop + pass = delta; every refusal.
// Stand-alone, built with -fsanitize=undefined,address by tests/test_band_filter_design_check.py.
#include "hostlogic/band_filter_design.hpp"

#include <complex>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace gr4pm::hostlogic;
typedef std::complex<double> cd;

static unsigned long long cases = 0, failures = 0;

#define CHECK(cond, ...)                                                                                                    \
    do {                                                                                                                    \
        if (!(cond)) {                                                                                                      \
            if (++failures <= 20) {                                                                                         \
                std::printf("FAILED %s (line %d): ", #cond, __LINE__);                                                      \
                std::printf(__VA_ARGS__);                                                                                   \
                std::printf("\n");                                                                                          \
            }                                                                                                               \
        }                                                                                                                   \
    } while (0)

static const double kPi = 3.14159265358979323846;
static const size_t kF = size_t(1) << 16;

// radix-2 decimation in time, forward sign, in place; the twiddles from a table made once
static void fft(std::vector<cd>& a)
{
    const size_t n = a.size();
    static std::vector<cd> tw;
    if (tw.size() != n / 2) {
        tw.resize(n / 2);
        for (size_t k = 0; k < n / 2; ++k) tw[k] = std::polar(1.0, -2.0 * kPi * static_cast<double>(k) / static_cast<double>(n));
    }
    for (size_t i = 1, j = 0; i < n; ++i) {
        size_t bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) std::swap(a[i], a[j]);
    }
    for (size_t len = 2; len <= n; len <<= 1)
        for (size_t i = 0; i < n; i += len)
            for (size_t k = 0; k < len / 2; ++k) {
                const cd u = a[i + k], v = a[i + k + len / 2] * tw[k * (n / len)];
                a[i + k] = u + v;
                a[i + k + len / 2] = u - v;
            }
}

static double circle_distance(double f, double e)
{
    double d = f - e;
    d -= std::floor(d + 0.5);
    return std::fabs(d);
}

static bool inside(const std::vector<MergedBand>& m, double f)
{
    for (const MergedBand& b : m)
        for (double shift : {-1.0, 0.0, 1.0})
            if (f + shift >= b.lo && f + shift <= b.hi) return true;
    return false;
}

// one design in one mode: the worst deviation from the ideal response outside the transitions, over 10^(-A / 20)
static void check_response(size_t L, double A, const std::vector<double>& bands, size_t merged_want)
{
    for (int pass = 0; pass < 2; ++pass) {
        ++cases;
        std::vector<double> taps;
        std::vector<MergedBand> m;
        const char* e = band_filter_design(bands.data(), bands.size() / 2, pass != 0, L, A, taps, &m);
        CHECK(!e, "L %zu A %g: refused: %s", L, A, e ? e : "");
        if (e) continue;
        CHECK(taps.size() == 2 * L && m.size() == merged_want, "L %zu: %zu taps, %zu merged bands", L, taps.size() / 2, m.size());
        std::vector<cd> H(kF, cd(0.0, 0.0));
        for (size_t t = 0; t < L; ++t) H[t] = cd(taps[2 * t], taps[2 * t + 1]);
        fft(H);
        const size_t c = (L - 1) / 2;
        const double half = 0.5 * band_filter_transition(L, A), ripple = std::pow(10.0, -A / 20.0);
        const double bound = 2.0 * static_cast<double>(m.size()) * ripple;
        double worst = 0.0;
        size_t checked = 0, in_band = 0;
        for (size_t k = 0; k < kF; ++k) {
            const double f = static_cast<double>(k) / static_cast<double>(kF);
            bool clear = true;
            for (const MergedBand& b : m)
                if (circle_distance(f, b.lo) < half || circle_distance(f, b.hi) < half) clear = false;
            if (!clear) continue;
            const bool in = inside(m, f);
            const double ideal = (in == (pass != 0)) ? 1.0 : 0.0;
            const cd rot = std::polar(1.0, 2.0 * kPi * static_cast<double>((k * c) % kF) / static_cast<double>(kF));
            worst = std::fmax(worst, std::abs(H[k] * rot - ideal));
            ++checked;
            in_band += in;
        }
        std::printf("L %zu A %g %s: %zu merged bands, worst deviation %.3f x 10^(-A/20) at %zu frequencies (%zu in a band)\n", L, A,
                    pass ? "pass" : "stop", m.size(), worst / ripple, checked, in_band);
        CHECK(worst <= bound, "L %zu A %g mode %d: deviation %g, bound %g", L, A, pass, worst, bound);
        CHECK(worst >= 0.1 * ripple, "L %zu A %g mode %d: deviation %g: the rule is vacuous here", L, A, pass, worst);
        CHECK(in_band > 0 && in_band < checked, "L %zu: both sides of an edge are checked", L);
    }
}

static std::vector<MergedBand> merged(const std::vector<double>& bands, const char** err = nullptr)
{
    std::vector<MergedBand> m;
    const char* e = band_filter_merge(bands.data(), bands.size() / 2, m);
    if (err) *err = e;
    return m;
}

static bool near(double a, double b) { return std::fabs(a - b) <= 1e-15; }

static void check_merging()
{
    ++cases;
    auto m = merged({0.1, 0.1, 0.15, 0.1}); // overlapping
    CHECK(m.size() == 1 && near(m[0].lo, 0.05) && near(m[0].hi, 0.2), "overlapping: %zu bands", m.size());
    ++cases;
    m = merged({0.25, 0.1, 0.1, 0.2}); // touching at 0.2, given in the other order
    CHECK(m.size() == 1 && near(m[0].lo, 0.0) && near(m[0].hi, 0.3), "touching: %zu bands [%g, %g]", m.size(), m[0].lo, m[0].hi);
    ++cases;
    m = merged({0.1, 0.05, 0.3, 0.05}); // apart
    CHECK(m.size() == 2 && near(m[0].lo, 0.075) && near(m[1].hi, 0.325), "apart: %zu bands", m.size());
    ++cases;
    m = merged({0.48, 0.1, -0.48, 0.1}); // both across +-0.5, overlapping there
    CHECK(m.size() == 1 && near(m[0].lo, 0.43) && near(m[0].hi, 0.57), "wrapping: %zu bands [%g, %g]", m.size(), m[0].lo, m[0].hi);
    ++cases;
    m = merged({-0.4, 0.2, 0.45, 0.2, 0.0, 0.1}); // [-0.5, -0.3] and [0.35, 0.55] meet round the circle; [-0.05, 0.05] stays
    CHECK(m.size() == 2 && near(m[0].lo, -0.05) && near(m[0].hi, 0.05) && near(m[1].lo, 0.35) && near(m[1].hi, 0.7),
          "round the circle: %zu bands", m.size());
    ++cases;
    m = merged({1.3, 0.1, -2.7, 0.1}); // centres folded: both are 0.3
    CHECK(m.size() == 1 && std::fabs(m[0].lo - 0.25) < 1e-12 && std::fabs(m[0].hi - 0.35) < 1e-12, "folded centres: %zu bands", m.size());
    ++cases;
    m = merged({});
    CHECK(m.empty(), "no bands");
    // the design of overlapping and wrapping bands is the design of what they merge to
    for (int pass = 0; pass < 2; ++pass) {
        ++cases;
        std::vector<double> a, b;
        const std::vector<double> two = {0.48, 0.1, -0.48, 0.1}, one = {0.5, 0.14};
        CHECK(!band_filter_design(two.data(), 2, pass != 0, 257, 60.0, a) && !band_filter_design(one.data(), 1, pass != 0, 257, 60.0, b),
              "refused");
        double worst = 0.0;
        for (size_t i = 0; i < a.size() && i < b.size(); ++i) worst = std::fmax(worst, std::fabs(a[i] - b[i]));
        CHECK(a.size() == b.size() && worst <= 1e-15, "merged design differs by %g", worst);
    }
}

static void check_complement()
{
    const std::vector<std::vector<double>> sets = {{0.05, 0.012}, {-0.3, 0.05, 0.12, 0.02, 0.49, 0.06}, {}};
    for (const auto& bands : sets)
        for (size_t L : {3u, 257u, 1025u}) {
            ++cases;
            std::vector<double> s, p;
            CHECK(!band_filter_design(bands.data(), bands.size() / 2, false, L, 60.0, s) &&
                      !band_filter_design(bands.data(), bands.size() / 2, true, L, 60.0, p),
                  "refused");
            double worst = 0.0;
            for (size_t t = 0; t < L; ++t) {
                worst = std::fmax(worst, std::fabs(s[2 * t] + p[2 * t] - (t == (L - 1) / 2 ? 1.0 : 0.0)));
                worst = std::fmax(worst, std::fabs(s[2 * t + 1] + p[2 * t + 1]));
            }
            CHECK(worst <= 1e-15, "L %zu: stop + pass differs from delta by %g", L, worst);
        }
}

static void refused(const std::vector<double>& bands, size_t L, double A, const char* word)
{
    ++cases;
    std::vector<double> taps;
    const char* e = band_filter_design(bands.data(), bands.size() / 2, false, L, A, taps);
    CHECK(e && std::strstr(e, word), "L %zu A %g: %s, expected a refusal about '%s'", L, A, e ? e : "accepted", word);
    CHECK(taps.empty(), "a refused design left taps");
}

static void check_refusals()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    refused({nan, 0.1}, 257, 60.0, "finite");
    refused({0.1, nan}, 257, 60.0, "finite");
    refused({inf, 0.1}, 257, 60.0, "finite");
    refused({0.1, -inf}, 257, 60.0, "finite");
    refused({0.1, 0.0}, 257, 60.0, "width");
    refused({0.1, -0.1}, 257, 60.0, "width");
    refused({0.1, 1.0}, 257, 60.0, "width");
    refused({0.1, 1.5}, 257, 60.0, "width");
    refused({0.1, 0.1}, 256, 60.0, "odd");
    refused({0.1, 0.1}, 1, 60.0, "odd");
    refused({0.1, 0.1}, 0, 60.0, "odd");
    refused({0.1, 0.1}, 2, 60.0, "odd");
    refused({0.1, 0.1}, 257, 8.0, "above 8");
    refused({0.1, 0.1}, 257, -60.0, "above 8");
    refused({0.1, 0.1}, 257, nan, "finite");
    refused({0.1, 0.1}, 257, inf, "finite");
    refused({0.0, 0.6, 0.5, 0.6}, 257, 60.0, "whole circle");
    refused({0.0, 0.5, 0.5, 0.5}, 257, 60.0, "whole circle"); // touching at both ends
    refused({-0.25, 0.3, 0.0, 0.3, 0.25, 0.3, 0.5, 0.3}, 257, 60.0, "whole circle");
}

int main()
{
    check_response(257, 60.0, {0.1, 0.2}, 1);
    check_response(1025, 60.0, {-0.3, 0.05, 0.12, 0.02, 0.49, 0.06}, 3); // the last one across +-0.5
    check_response(1025, 40.0, {0.0, 0.006}, 1);
    check_response(513, 80.0, {-0.2, 0.1, 0.25, 0.08}, 2);
    check_merging();
    check_complement();
    check_refusals();
    std::printf("band_filter_design_check: %llu cases, %llu failures\n", cases, failures);
    return failures ? 1 : 0;
}
