// hostlogic/carrier_find.hpp -- carriers from a power spectrum (gr4pm_find_carriers), HIP-free and host only.
//
// psd: n bins in FFT order (bin k is the frequency k / n, k > n / 2: negative frequencies), a circle.
//   1. floor = the lower median: element (n - 1) / 2 of the sorted copy.
//   2. bin k is occupied iff psd[k] > floor 10^(threshold_db / 10).
//   3. runs of occupied bins on the circle; runs that at most max_gap_bins free bins separate merge (the free bins
//      between them belong to the merged run); then runs shorter than min_width_bins are dropped.  The walk starts
//      behind the longest stretch of free bins (of several, the one that begins at the lowest bin), so no run is cut.
//   4. a run of len bins from bin a, i = 0 .. len - 1 over the bins (a + i) mod n, in double, in index order:
//        c = sum i (psd - floor) / sum (psd - floor),  frequency = (a + c) / n folded to [-0.5, 0.5),
//        bandwidth = len / n,  power = sum (psd - floor),  snr_db = 10 log10(max psd / floor)
//   5. ascending frequency.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../../include/gr4pm_hip.h"

namespace gr4pm {
namespace hostlogic {

using Carrier = gr4pm_carrier; // frequency, bandwidth, power, snr_db, first_bin, n_bins

inline double lower_median(const double* psd, size_t n)
{
    std::vector<double> s(psd, psd + n);
    std::nth_element(s.begin(), s.begin() + (n - 1) / 2, s.end());
    return s[(n - 1) / 2];
}

// every carrier, in ascending frequency; n >= 1, threshold_db > 0
inline std::vector<Carrier> find_carriers(const double* psd, size_t n, double threshold_db, size_t max_gap_bins,
                                          size_t min_width_bins)
{
    std::vector<Carrier> found;
    const double floor_ = lower_median(psd, n);
    const double level = floor_ * std::pow(10.0, threshold_db / 10.0);
    std::vector<unsigned char> occ(n);
    size_t n_occ = 0;
    for (size_t k = 0; k < n; ++k) n_occ += (occ[k] = psd[k] > level ? 1 : 0);
    if (n_occ == 0 || n_occ == n) return found; // (all occupied cannot happen with a positive threshold and a finite PSD)
    // the longest stretch of free bins, the first of equals by its first bin
    size_t best_start = 0, best_len = 0;
    for (size_t k = 0; k < n; ++k) {
        if (occ[k] || !occ[(k + n - 1) % n]) continue; // k begins a stretch
        size_t len = 0;
        while (!occ[(k + len) % n]) ++len;
        if (len > best_len) best_len = len, best_start = k;
    }
    const size_t p0 = (best_start + best_len) % n; // occupied; the n - best_len bins from here end on an occupied bin
    const size_t span = n - best_len;
    size_t i = 0;
    while (i < span) {
        // a run begins at p0 + i (occupied)
        size_t last = i, j = i + 1;
        while (j < span) {
            if (occ[(p0 + j) % n]) {
                last = j++;
                continue;
            }
            size_t gap = 0;
            while (!occ[(p0 + j + gap) % n]) ++gap; // ends: bin p0 + span - 1 is occupied
            if (gap > max_gap_bins) break;
            j += gap;
        }
        const size_t a = (p0 + i) % n, len = last - i + 1;
        if (len >= min_width_bins) {
            double num = 0.0, den = 0.0, peak = psd[a];
            for (size_t t = 0; t < len; ++t) {
                const double v = psd[(a + t) % n];
                num += static_cast<double>(t) * (v - floor_);
                den += v - floor_;
                peak = v > peak ? v : peak;
            }
            double f = (static_cast<double>(a) + num / den) / static_cast<double>(n);
            f -= std::floor(f + 0.5);
            found.push_back(Carrier{f, static_cast<double>(len) / static_cast<double>(n), den, 10.0 * std::log10(peak / floor_),
                                    a, len});
        }
        // the next run begins behind the gap that ended this one
        i = last + 1;
        while (i < span && !occ[(p0 + i) % n]) ++i;
    }
    std::stable_sort(found.begin(), found.end(), [](const Carrier& x, const Carrier& y) { return x.frequency < y.frequency; });
    return found;
}

// the ABI's form: the first min(cap, count) carriers to out[0 .. cap), returns the count
inline size_t find_carriers(const double* psd, size_t n, double threshold_db, size_t max_gap_bins, size_t min_width_bins,
                            Carrier* out, size_t cap)
{
    const std::vector<Carrier> found = find_carriers(psd, n, threshold_db, max_gap_bins, min_width_bins);
    for (size_t i = 0; i < found.size() && i < cap; ++i) out[i] = found[i];
    return found.size();
}

} // namespace hostlogic
} // namespace gr4pm
