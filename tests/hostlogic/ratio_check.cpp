// ratio_check.cpp -- csrc/hostlogic/ratio.hpp (gr4pm_simplest_ratio) as a stand-alone program for
// -fsanitize=undefined,address: the Stern-Brocot walk against brute force over every denominator <= 1024 (the smallest
// admissible numerator of each, in ascending order of the denominator) for a few hundred values and three tolerances, with
// wide and with narrow maxima; the result is in lowest terms and inside the interval by the walk's own comparison.
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include <numeric>

#include "hostlogic/ratio.hpp"

using namespace gr4pm::hostlogic;

static long g_cases = 0, g_failures = 0;

static bool brute(double value, double tol, uint32_t max_num, uint32_t max_den, uint32_t* num, uint32_t* den)
{
    const double lo = value * (1.0 - tol), hi = value * (1.0 + tol);
    for (uint32_t q = 1; q <= max_den; ++q) {
        for (uint32_t p = 1; p <= max_num; ++p) {
            const double pf = p, qf = q;
            if (pf < lo * qf) continue;
            if (pf > hi * qf) break;
            *num = p, *den = q;
            return true;
        }
    }
    return false;
}

static void check(double value, double tol, uint32_t max_num, uint32_t max_den)
{
    ++g_cases;
    uint32_t p = 0, q = 0, bp = 0, bq = 0;
    const bool got = simplest_ratio(value, tol, max_num, max_den, &p, &q), want = brute(value, tol, max_num, max_den, &bp, &bq);
    bool ok = got == want;
    if (got && want) ok = p == bp && q == bq && std::gcd(p, q) == 1u && p <= max_num && q <= max_den;
    if (!ok) {
        ++g_failures;
        std::printf("FAIL value %.17g tol %g max %u / %u: walk %d %u/%u, brute force %d %u/%u\n", value, tol, max_num, max_den, got, p,
                    q, want, bp, bq);
    }
}

int main()
{
    uint64_t state = 12345;
    auto uniform = [&] { // a 53-bit fraction from a 64-bit LCG
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return static_cast<double>(state >> 11) / 9007199254740992.0;
    };
    for (int i = 0; i < 300; ++i) {
        const double value = std::exp(std::log(1e-3) + uniform() * (std::log(64.0) - std::log(1e-3)));
        for (double tol : {2e-3, 1e-5, 0.05}) {
            check(value, tol, 64, 1024);
            check(value, tol, 7, 9);
        }
    }
    for (double value : {0.16, 4.0 / 25.0, 1.0 / 3.0, 1.0, 0.5, 64.0, 1.0 / 1024.0, 1.0 / 1025.0, 65.0, 0.999, 63.0 / 1024.0})
        for (double tol : {0.0, 2e-3, 1e-9}) check(value, tol, 64, 1024);
    if (!ratio_arguments_valid(0.5, 0.0, 1, 1) || ratio_arguments_valid(0.0, 0.1, 1, 1) || ratio_arguments_valid(-1.0, 0.1, 1, 1) ||
        ratio_arguments_valid(NAN, 0.1, 1, 1) || ratio_arguments_valid(INFINITY, 0.1, 1, 1) || ratio_arguments_valid(0.5, -0.1, 1, 1) ||
        ratio_arguments_valid(0.5, 1.0, 1, 1) || ratio_arguments_valid(0.5, NAN, 1, 1) || ratio_arguments_valid(0.5, 0.1, 0, 1) ||
        ratio_arguments_valid(0.5, 0.1, 1, 0)) {
        ++g_failures;
        std::printf("FAIL ratio_arguments_valid\n");
    }
    ++g_cases;
    std::printf("ratio_check: %ld cases, %ld failures\n", g_cases, g_failures);
    return g_failures ? 1 : 0;
}
