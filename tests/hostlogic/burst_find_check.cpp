// burst_find_check.cpp -- csrc/hostlogic/burst_find.hpp (what gr4pm_find_bursts runs) as a stand-alone program for
// -fsanitize=undefined,address: synthetic power series with room for all bursts, for one and for none; runs at row 0 and
// at the last row; gaps of max_gap_rows and one more; max_gap_rows and min_rows at 0 and at SIZE_MAX; a series of one row.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hostlogic/burst_find.hpp"

using namespace gr4pm::hostlogic;

static unsigned long long g_cases = 0, g_failures = 0;

#define CHECK(cond)                                                                                                   \
    do {                                                                                                              \
        if (!(cond)) {                                                                                                \
            if (g_failures++ < 20) std::printf("FAIL %s (case %llu) line %d\n", #cond, g_cases, __LINE__);            \
        }                                                                                                             \
    } while (0)

struct Run {
    size_t first, len;
};

static std::vector<double> series(size_t T, const std::vector<Run>& runs)
{
    std::vector<double> p(T);
    for (size_t t = 0; t < T; ++t) p[t] = 1.0 + 0.001 * static_cast<double>((t * 7919) % 13);
    for (const Run& r : runs)
        for (size_t t = r.first; t < r.first + r.len; ++t) p[t] = 30.0 + static_cast<double>((t * 31) % 7);
    return p;
}

// the finder with room for every burst, for one and for none: the same bursts, the same count
static std::vector<Burst> run_case(const std::vector<double>& p, double thr, double floor_in, size_t gap, size_t min_rows,
                                   const std::vector<Run>& want)
{
    ++g_cases;
    std::vector<Burst> all(p.size() + 1);
    const size_t count = find_bursts(p.data(), p.size(), thr, floor_in, gap, min_rows, all.data(), all.size());
    CHECK(count == want.size());
    all.resize(count < all.size() ? count : all.size());
    for (size_t i = 0; i < all.size() && i < want.size(); ++i) {
        CHECK(all[i].first_row == want[i].first && all[i].n_rows == want[i].len);
        CHECK(all[i].peak_row >= all[i].first_row && all[i].peak_row < all[i].first_row + all[i].n_rows);
        CHECK(all[i].power > 0.0 && all[i].snr_db > thr);
        if (i) CHECK(all[i].first_row > all[i - 1].first_row + all[i - 1].n_rows);
    }
    Burst one[1];
    CHECK(find_bursts(p.data(), p.size(), thr, floor_in, gap, min_rows, one, 1) == count);
    if (count) CHECK(one[0].first_row == all[0].first_row && one[0].n_rows == all[0].n_rows);
    CHECK(find_bursts(p.data(), p.size(), thr, floor_in, gap, min_rows, nullptr, 0) == count);
    return all;
}

int main()
{
    const size_t big = static_cast<size_t>(-1);
    run_case(series(200, {}), 6.0, 0.0, 1, 2, {});
    run_case(std::vector<double>(50, 2.5), 6.0, 0.0, 1, 2, {});
    run_case(series(200, {{60, 9}}), 6.0, 0.0, 1, 2, {{60, 9}});
    run_case(series(300, {{20, 5}, {100, 17}, {250, 3}}), 6.0, 0.0, 1, 2, {{20, 5}, {100, 17}, {250, 3}});
    run_case(series(200, {{40, 5}, {47, 5}}), 6.0, 0.0, 2, 2, {{40, 12}});          // a gap of max_gap_rows merges
    run_case(series(200, {{40, 5}, {48, 5}}), 6.0, 0.0, 2, 2, {{40, 5}, {48, 5}}); // one more does not
    run_case(series(200, {{40, 5}, {46, 5}}), 6.0, 0.0, 0, 2, {{40, 5}, {46, 5}});
    run_case(series(200, {{30, 3}, {90, 4}}), 6.0, 0.0, 1, 4, {{90, 4}});          // min_rows - 1 is dropped
    run_case(series(200, {{30, 1}, {32, 1}}), 6.0, 0.0, 1, 3, {{30, 3}});          // the bridged row counts
    run_case(series(200, {{0, 6}}), 6.0, 0.0, 1, 2, {{0, 6}});
    run_case(series(200, {{193, 7}}), 6.0, 0.0, 1, 2, {{193, 7}});
    run_case(series(120, {{0, 4}, {116, 4}}), 6.0, 0.0, 1, 2, {{0, 4}, {116, 4}});
    run_case(series(120, {{0, 4}, {116, 4}}), 6.0, 0.0, big, 0, {{0, 120}});        // every gap merges, no overflow
    run_case(series(120, {{0, 4}, {116, 4}}), 6.0, 0.0, 1, big, {});
    run_case(series(100, {{5, 30}, {50, 35}}), 6.0, 0.0, 1, 2, {});                 // the median is a burst row
    run_case(series(100, {{5, 30}, {50, 35}}), 6.0, 1.02, 1, 2, {{5, 30}, {50, 35}}); // an explicit floor
    run_case(std::vector<double>(1, 3.0), 6.0, 0.0, 1, 1, {});
    run_case(std::vector<double>(1, 3.0), 6.0, 0.5, 1, 1, {{0, 1}});
    { // the values of one burst, worked out by hand: rows 2 .. 6 with row 5 bridged
        const std::vector<double> p = {1.0, 1.0, 11.0, 21.0, 21.0, 1.0, 5.0, 1.0, 1.0, 1.0, 1.0};
        const std::vector<Burst> b = run_case(p, 3.0, 0.0, 1, 2, {{2, 5}});
        if (b.size() == 1) {
            CHECK(b[0].peak_row == 3);
            CHECK(b[0].power == (10.0 + 20.0 + 20.0 + 0.0 + 4.0) / 5.0);
            CHECK(std::fabs(b[0].snr_db - 10.0 * std::log10(21.0)) < 1e-12);
        }
    }
    std::printf("burst_find_check: %llu cases, %llu failures\n", g_cases, g_failures);
    return g_failures ? 1 : 0;
}
