// hostlogic/burst_find.hpp -- bursts from a band's power over time (gr4pm_find_bursts), HIP-free and host only; the
// sibling of carrier_find.hpp on the time axis.
//
// p: T rows in time order (a line, not a circle: nothing wraps).
//   1. floor = the caller's value if > 0, else the lower median: element (T - 1) / 2 of the sorted copy.
//   2. row t is active iff p[t] > floor 10^(threshold_db / 10).
//   3. runs of active rows in time order; runs that at most max_gap_rows inactive rows separate merge (the inactive rows
//      between them belong to the merged run); then runs shorter than min_rows are dropped.
//   4. a run of len rows from row a, over t = a .. a + len - 1 in double, in index order:
//        power = sum (p - floor) / len,  peak_row = the first row of the maximum,  snr_db = 10 log10(peak / floor)
//   5. ascending time.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../../include/gr4pm_hip.h"
#include "carrier_find.hpp"

namespace gr4pm {
namespace hostlogic {

using Burst = gr4pm_burst; // first_row, n_rows, peak_row, power, snr_db

// every burst, in ascending time; T >= 1, threshold_db > 0, floor_in >= 0 and finite (0: the lower median)
inline std::vector<Burst> find_bursts(const double* p, size_t T, double threshold_db, double floor_in, size_t max_gap_rows,
                                      size_t min_rows)
{
    std::vector<Burst> found;
    const double floor_ = floor_in > 0.0 ? floor_in : lower_median(p, T);
    const double level = floor_ * std::pow(10.0, threshold_db / 10.0);
    size_t t = 0;
    while (t < T) {
        if (!(p[t] > level)) {
            ++t;
            continue;
        }
        // a run begins at t; it goes on across stretches of at most max_gap_rows inactive rows that an active row ends
        size_t last = t, j = t + 1, gap = 0;
        for (; j < T; ++j) {
            if (p[j] > level) {
                last = j;
                gap = 0;
            } else if (++gap > max_gap_rows) {
                break;
            }
        }
        const size_t len = last - t + 1;
        if (len >= min_rows) {
            double sum = 0.0, peak = p[t];
            size_t peak_row = t;
            for (size_t i = t; i <= last; ++i) {
                sum += p[i] - floor_;
                if (p[i] > peak) peak = p[i], peak_row = i;
            }
            found.push_back(Burst{t, len, peak_row, sum / static_cast<double>(len), 10.0 * std::log10(peak / floor_)});
        }
        t = last + 1;
    }
    return found;
}

// the ABI's form: the first min(cap, count) bursts to out[0 .. cap), returns the count
inline size_t find_bursts(const double* p, size_t T, double threshold_db, double floor_in, size_t max_gap_rows, size_t min_rows,
                          Burst* out, size_t cap)
{
    const std::vector<Burst> found = find_bursts(p, T, threshold_db, floor_in, max_gap_rows, min_rows);
    for (size_t i = 0; i < found.size() && i < cap; ++i) out[i] = found[i];
    return found.size();
}

} // namespace hostlogic
} // namespace gr4pm
