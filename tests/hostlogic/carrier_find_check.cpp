// carrier_find_check.cpp -- csrc/hostlogic/carrier_find.hpp (gr4pm_find_carriers) as a stand-alone program for
// -fsanitize=undefined,address: synthetic spectra (one carrier, three, a carrier across +-0.5 and across bin 0, gaps of
// max_gap_bins and max_gap_bins + 1, a run of min_width_bins - 1, flat, all bins equal but one, n = 1 and an odd n) with
// room for every carrier, for one (cap = 1) and for none (cap = 0, out == nullptr): the heap blocks have exactly cap items.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "hostlogic/carrier_find.hpp"

using namespace gr4pm::hostlogic;

static int g_failures = 0, g_cases = 0;

static void block(std::vector<double>& p, size_t first, size_t len, double v)
{
    for (size_t i = 0; i < len; ++i) p[(first + i) % p.size()] = v + 0.25 * static_cast<double>(i % 3);
}

struct Want {
    size_t first, len;
};

static void run(const char* name, const std::vector<double>& psd, size_t gap, size_t width, std::vector<Want> want)
{
    ++g_cases;
    const size_t n = psd.size();
    const std::vector<Carrier> all = find_carriers(psd.data(), n, 6.0, gap, width);
    bool ok = all.size() == want.size();
    for (size_t i = 0; ok && i < all.size(); ++i) {
        bool hit = false;
        for (const Want& w : want) hit = hit || (all[i].first_bin == w.first && all[i].n_bins == w.len);
        ok = hit && all[i].frequency >= -0.5 && all[i].frequency < 0.5 && (i == 0 || all[i - 1].frequency < all[i].frequency) &&
             all[i].power > 0.0 && all[i].bandwidth == static_cast<double>(all[i].n_bins) / static_cast<double>(n);
    }
    for (size_t cap : {size_t(0), size_t(1), all.size()}) {
        std::unique_ptr<Carrier[]> out(cap ? new Carrier[cap] : nullptr);
        const size_t count = find_carriers(psd.data(), n, 6.0, gap, width, out.get(), cap);
        ok = ok && count == all.size();
        for (size_t i = 0; i < cap && i < count; ++i) ok = ok && std::memcmp(&out[i], &all[i], sizeof(Carrier)) == 0;
    }
    if (!ok) {
        ++g_failures;
        std::printf("FAIL %s: %zu carriers, wanted %zu\n", name, all.size(), want.size());
        for (const Carrier& c : all)
            std::printf("   first %llu len %llu f %.6f\n", (unsigned long long)c.first_bin, (unsigned long long)c.n_bins, c.frequency);
    }
}

int main()
{
    const size_t n = 2048;
    const std::vector<double> flat(n, 1.0);
    std::vector<double> p;
    p = flat, block(p, 300, 41, 30.0);
    run("one", p, 2, 4, {{300, 41}});
    p = flat, block(p, 1400, 60, 12.0), block(p, 260, 31, 100.0), block(p, 900, 45, 40.0);
    run("three", p, 2, 4, {{1400, 60}, {260, 31}, {900, 45}});
    p = flat, block(p, 999, 50, 25.0);
    run("across +-0.5", p, 2, 4, {{999, 50}});
    p = flat, block(p, 2031, 40, 25.0);
    run("across bin 0", p, 2, 4, {{2031, 40}});
    p = flat, block(p, 100, 10, 50.0), block(p, 112, 10, 60.0);
    run("gap of max_gap_bins", p, 2, 4, {{100, 22}});
    p = flat, block(p, 100, 10, 50.0), block(p, 113, 10, 60.0);
    run("gap of max_gap_bins + 1", p, 2, 4, {{100, 10}, {113, 10}});
    p = flat, block(p, 2046, 3, 50.0), block(p, 3, 5, 60.0); // the gap of two spans bins 1 and 2
    run("a merged run across bin 0", p, 2, 4, {{2046, 10}});
    p = flat, block(p, 500, 3, 40.0), block(p, 700, 4, 40.0);
    run("run of min_width_bins - 1", p, 2, 4, {{700, 4}});
    run("flat", flat, 2, 4, {});
    p = flat, p[77] = 100.0;
    run("one bin", p, 0, 1, {{77, 1}});
    run("one bin, too narrow", p, 0, 2, {});
    p = flat, block(p, 0, 1023, 9.0); // just under half of the band
    run("almost half", p, 0, 1, {{0, 1023}});
    run("n = 1", std::vector<double>(1, 2.0), 2, 4, {});
    p.assign(257, 1.0), block(p, 250, 10, 9.0), block(p, 120, 11, 20.0);
    run("odd n", p, 2, 4, {{250, 10}, {120, 11}});
    p.assign(8, 0.0), p[3] = 1.0, p[4] = 2.0; // a floor of zero: everything above it is occupied
    run("zero floor", p, 0, 1, {{3, 2}});
    std::printf("carrier_find_check: %d cases, %d failures\n", g_cases, g_failures);
    return g_failures ? 1 : 0;
}
