// hostlogic/ratio.hpp -- the simplest fraction near a value (gr4pm_simplest_ratio), HIP-free and host only.
//
// lo = value (1 - rel_tol), hi = value (1 + rel_tol), both in double.  num / den lies inside iff
// double(num) >= lo * double(den) and double(num) <= hi * double(den).  The walk descends the Stern-Brocot tree from
// 0/1 and 1/0 in integers: the mediant goes right while it lies below lo and left while it lies above hi; the first
// mediant inside [lo, hi] is the fraction of the interval with the smallest denominator AND the smallest numerator (every
// other fraction of the interval descends from it), and it is in lowest terms.  If it exceeds max_num or max_den, so does
// every other, and there is none.  At most max_num + max_den steps.
#pragma once
#include <cmath>
#include <cstdint>

namespace gr4pm {
namespace hostlogic {

inline bool ratio_arguments_valid(double value, double rel_tol, uint32_t max_num, uint32_t max_den)
{
    return std::isfinite(value) && std::isfinite(rel_tol) && value > 0.0 && rel_tol >= 0.0 && rel_tol < 1.0 && max_num >= 1 &&
           max_den >= 1;
}

// ratio_arguments_valid() holds; false: no such fraction
inline bool simplest_ratio(double value, double rel_tol, uint32_t max_num, uint32_t max_den, uint32_t* num, uint32_t* den)
{
    const double lo = value * (1.0 - rel_tol), hi = value * (1.0 + rel_tol);
    uint64_t a = 0, b = 1, c = 1, d = 0; // a / b < the interval < c / d
    for (;;) {
        const uint64_t p = a + c, q = b + d;
        if (p > max_num || q > max_den) return false;
        const double pf = static_cast<double>(p), qf = static_cast<double>(q);
        if (pf < lo * qf)
            a = p, b = q;
        else if (pf > hi * qf)
            c = p, d = q;
        else {
            *num = static_cast<uint32_t>(p), *den = static_cast<uint32_t>(q);
            return true;
        }
    }
}

} // namespace hostlogic
} // namespace gr4pm
