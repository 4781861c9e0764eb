// hostlogic/band_filter_design.hpp -- the designer behind gr4pm_band_filter_taps (fft_filter.hip),
// HIP-free and in double: complex taps that stop or pass a set of bands of a complex stream.
//
// A band is (centre, width) in cycles per sample, anywhere on the circle of frequencies (period 1): it may wrap across
// +-0.5.  Bands that overlap or touch are merged on the circle first.  With n_taps odd, c = (n_taps - 1) / 2, w the Kaiser
// window whose beta follows from attenuation_db by the rule of kaiser_design.hpp, and per merged band [f_lo, f_hi]
//     g_b(m) = (e^{2 pi j f_hi m} - e^{2 pi j f_lo m}) / (2 pi j m),   g_b(0) = f_hi - f_lo
//            = e^{2 pi j fc m} sin(pi width m) / (pi m)   (the form evaluated: no difference of nearly equal phasors)
// the taps are
//     pass:  h[t] = w[t] sum_b g_b(t - c)
//     stop:  h[t] = w[t] (delta[t - c] - sum_b g_b(t - c))
// so that H(f) e^{2 pi j f c} is 1 inside the bands (pass) or outside them (stop) and 0 elsewhere, up to the window's
// ripple 10^(-A / 20) per band edge, beyond half a transition width (A - 7.95) / (14.36 (n_taps - 1)) from an edge.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace gr4pm {
namespace hostlogic {

struct MergedBand {
    double lo, hi; // lo in [-0.5, 0.5), lo < hi < lo + 1
};

// the transition width of a design, in cycles per sample
inline double band_filter_transition(size_t n_taps, double attenuation_db)
{
    return (attenuation_db - 7.95) / (14.36 * static_cast<double>(n_taps - 1));
}

// bands: n pairs (centre, width).  The merged bands in ascending lo; NULL, or the text of the refusal
inline const char* band_filter_merge(const double* bands, size_t n, std::vector<MergedBand>& out)
{
    out.clear();
    if (n && !bands) return "no bands array";
    std::vector<MergedBand> v;
    v.reserve(n);
    for (size_t b = 0; b < n; ++b) {
        const double centre = bands[2 * b], width = bands[2 * b + 1];
        if (!std::isfinite(centre) || !std::isfinite(width)) return "a band's centre or width is not finite";
        if (!(width > 0.0) || !(width < 1.0)) return "a band's width must lie inside (0, 1)";
        double lo = centre - 0.5 * width;
        lo -= std::floor(lo + 0.5); // to [-0.5, 0.5)
        if (lo >= 0.5) lo -= 1.0;   // (a rounding at the edge)
        v.push_back(MergedBand{lo, lo + width});
    }
    std::sort(v.begin(), v.end(), [](const MergedBand& a, const MergedBand& b) { return a.lo < b.lo; });
    for (const MergedBand& b : v) {
        if (!out.empty() && b.lo <= out.back().hi)
            out.back().hi = std::max(out.back().hi, b.hi);
        else
            out.push_back(b);
    }
    // round the circle: the last band may reach the first one (and, through it, further ones)
    while (out.size() > 1 && out.back().hi >= out.front().lo + 1.0) {
        MergedBand last = out.back();
        last.hi = std::max(last.hi, out.front().hi + 1.0);
        out.pop_back();
        out.erase(out.begin());
        out.push_back(last);
    }
    for (const MergedBand& b : out)
        if (b.hi - b.lo >= 1.0) return "the bands cover the whole circle";
    std::sort(out.begin(), out.end(), [](const MergedBand& a, const MergedBand& b) { return a.lo < b.lo; });
    return nullptr;
}

inline double band_filter_kaiser_beta(double A)
{
    return A > 50.0 ? 0.1102 * (A - 8.7) : (A >= 21.0 ? 0.5842 * std::pow(A - 21.0, 0.4) + 0.07886 * (A - 21.0) : 0.0);
}

// taps: n_taps pairs (re, im) in double.  NULL, or the text of the refusal (taps then holds nothing of use).  merged: the
// bands the design was made for, when the caller wants them
inline const char* band_filter_design(const double* bands, size_t n_bands, bool pass, size_t n_taps, double attenuation_db,
                                      std::vector<double>& taps, std::vector<MergedBand>* merged = nullptr)
{
    taps.clear();
    if (n_taps < 3 || n_taps % 2 == 0) return "n_taps must be odd and at least 3";
    if (!std::isfinite(attenuation_db)) return "attenuation_db is not finite";
    if (!(attenuation_db > 8.0)) return "attenuation_db must be above 8";
    std::vector<MergedBand> m;
    if (const char* e = band_filter_merge(bands, n_bands, m)) return e;
    const double pi = 3.14159265358979323846;
    const double beta = band_filter_kaiser_beta(attenuation_db);
    const double i0b = std::cyl_bessel_i(0.0, beta);
    const double c = 0.5 * static_cast<double>(n_taps - 1);
    taps.assign(2 * n_taps, 0.0);
    for (size_t t = 0; t < n_taps; ++t) {
        const double k = static_cast<double>(t) - c; // an integer: n_taps is odd
        const double u = k / c;
        const double w = std::cyl_bessel_i(0.0, beta * std::sqrt(std::fmax(0.0, 1.0 - u * u))) / i0b;
        double re = 0.0, im = 0.0;
        for (const MergedBand& b : m) {
            const double width = b.hi - b.lo, fc = 0.5 * (b.lo + b.hi);
            if (k == 0.0) {
                re += width;
                continue;
            }
            // the phases reduced to a turn before they meet pi: k is an integer, so fc k mod 1 and width k mod 2 lose nothing
            const double a = std::sin(pi * std::fmod(width * k, 2.0)) / (pi * k);
            const double ph = 2.0 * pi * std::fmod(fc * k, 1.0);
            re += a * std::cos(ph);
            im += a * std::sin(ph);
        }
        if (!pass) {
            re = (k == 0.0 ? 1.0 : 0.0) - re;
            im = -im;
        }
        taps[2 * t] = w * re;
        taps[2 * t + 1] = w * im;
    }
    if (merged) *merged = m;
    return nullptr;
}

} // namespace hostlogic
} // namespace gr4pm
