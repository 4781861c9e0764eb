// kaiser_design.hpp -- the prototype low-pass of the Channelizer (channelizer.hip), the Ddc (ddc.hip) and the Duc
// (duc.hip): host only.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

namespace gr4pm {

// the band edges a design takes for a decimation by D: 0 <= passband < stopband and the cutoff, midway between them,
// below fs / 2, or at most fs / 2 where `cutoff_at_nyquist` (the Ddc and the Duc; the Channelizer does not allow it).
// A NaN fails.
inline bool band_edges_valid(double passband, double stopband, size_t D, bool cutoff_at_nyquist)
{
    const double sum = passband + stopband, d = static_cast<double>(D);
    return passband >= 0.0 && passband < stopband && (cutoff_at_nyquist ? sum <= d : sum < d);
}

// Kaiser-windowed sinc of L taps in double for a decimation by D: band edges in units of the output rate fs / D, the
// cutoff midway between them, the window's beta from the attenuation that Kaiser's length rule gives for L taps over
// the transition width; DC gain 1, or `gain` (an interpolator's D), applied in double to the unit-gain taps.  The caller
// has checked L >= 1, D >= 1 and 0 <= passband < stopband.
inline void kaiser_lowpass(size_t L, size_t D, double passband, double stopband, std::vector<double>& h, double gain = 1.0)
{
    const double pi = 3.14159265358979323846;
    const double dw = 2.0 * pi * (stopband - passband) / static_cast<double>(D);
    const double A = 2.285 * dw * static_cast<double>(L - 1) + 7.95;
    const double beta = A > 50.0 ? 0.1102 * (A - 8.7)
                                 : (A >= 21.0 ? 0.5842 * std::pow(A - 21.0, 0.4) + 0.07886 * (A - 21.0) : 0.0);
    const double fc = 0.5 * (passband + stopband) / static_cast<double>(D); // cycles per input sample
    const double centre = 0.5 * static_cast<double>(L - 1);
    const double i0b = std::cyl_bessel_i(0.0, beta);
    h.assign(L, 0.0);
    double sum = 0.0;
    for (size_t t = 0; t < L; ++t) {
        // one tap: the window is 1 (u would be 0 / 0)
        const double u = L > 1 ? 2.0 * static_cast<double>(t) / static_cast<double>(L - 1) - 1.0 : 0.0;
        const double w = std::cyl_bessel_i(0.0, beta * std::sqrt(std::fmax(0.0, 1.0 - u * u))) / i0b;
        const double x = 2.0 * fc * (static_cast<double>(t) - centre);
        const double sinc = x == 0.0 ? 1.0 : std::sin(pi * x) / (pi * x);
        h[t] = 2.0 * fc * sinc * w;
        sum += h[t];
    }
    for (double& v : h) v /= sum;
    if (gain != 1.0)
        for (double& v : h) v *= gain;
}

} // namespace gr4pm
