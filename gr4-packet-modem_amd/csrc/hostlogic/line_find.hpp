// hostlogic/line_find.hpp -- the line of a spectrum (gr4pm_find_line), HIP-free and host only.
//
// spectrum: n bins in FFT order, a circle.  The window is the bins (first_bin + i) mod n, i = 0 .. n_bins - 1, with
// first_bin < n and 2 guard_bins + 3 <= n_bins <= n.
//   1. peak = the first maximum in window order, at `bin`.
//   2. floor = the lower median of the window's bins: element (n_bins - 1) / 2 of the sorted copy.
//   3. snr_db = 10 log10(peak / floor).
//   4. margin_db = 10 log10(peak / other), other = the largest window bin whose circular distance to `bin`,
//      min(|k - bin|, n - |k - bin|), is above guard_bins (n_bins >= 2 guard_bins + 3: there are at least two).
//   5. la, lb, lc = ln of the bins bin - 1, bin, bin + 1 on the circle (inside the window or not);
//      d = 0.5 (la - lc) / (la - 2 lb + lc) clamped to +-0.5, d = 0 if any of the three bins is <= 0 or the curvature is
//      not negative; frequency = (bin + d) / n folded to [-0.5, 0.5).
//   6. found = peak > 0; without it snr_db = margin_db = 0 and d = 0.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../../include/gr4pm_hip.h"

namespace gr4pm {
namespace hostlogic {

using Line = gr4pm_line; // frequency, snr_db, margin_db, peak, floor, bin, found

inline bool line_window_valid(size_t n, uint64_t first_bin, uint64_t n_bins, uint64_t guard_bins)
{
    return n > 0 && first_bin < n && n_bins <= n && guard_bins <= (UINT64_MAX - 3) / 2 && n_bins >= 2 * guard_bins + 3;
}

// line_window_valid() holds
inline Line find_line(const double* sp, size_t n, uint64_t first_bin, uint64_t n_bins, uint64_t guard_bins)
{
    Line out = {};
    std::vector<double> win(n_bins);
    size_t ip = 0;
    for (size_t i = 0; i < n_bins; ++i) {
        win[i] = sp[(first_bin + i) % n];
        if (win[i] > win[ip]) ip = i;
    }
    const size_t bin = (first_bin + ip) % n;
    const double peak = win[ip];
    double other = 0.0;
    bool have_other = false;
    for (size_t i = 0; i < n_bins; ++i) {
        const size_t k = (first_bin + i) % n;
        const size_t d = k > bin ? k - bin : bin - k;
        const size_t dist = d < n - d ? d : n - d;
        if (dist <= guard_bins) continue;
        if (!have_other || win[i] > other) other = win[i], have_other = true;
    }
    std::nth_element(win.begin(), win.begin() + (n_bins - 1) / 2, win.end());
    out.floor = win[(n_bins - 1) / 2];
    out.peak = peak;
    out.bin = bin;
    out.found = peak > 0.0 ? 1 : 0;
    double d = 0.0;
    if (out.found) {
        out.snr_db = 10.0 * std::log10(peak / out.floor);
        out.margin_db = 10.0 * std::log10(peak / other);
        const double a = sp[(bin + n - 1) % n], c = sp[(bin + 1) % n];
        if (a > 0.0 && c > 0.0) {
            const double la = std::log(a), lb = std::log(peak), lc = std::log(c);
            const double curv = la - 2.0 * lb + lc;
            if (curv < 0.0) {
                d = 0.5 * (la - lc) / curv;
                d = d > 0.5 ? 0.5 : d < -0.5 ? -0.5 : d;
            }
        }
    }
    double f = (static_cast<double>(bin) + d) / static_cast<double>(n);
    f -= std::floor(f + 0.5);
    out.frequency = f;
    return out;
}

} // namespace hostlogic
} // namespace gr4pm
