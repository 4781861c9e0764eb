// Sweeps csrc/hostlogic/fft_filter_plan.hpp (the FftFilter's host side) against restatements in
// __int128 from "segment s is the N items from s hop - V" alone: every refusal of the validation (each must occur), the
// default overlap, and for a set of overlaps the segments, carried samples, first output index and reads of sequences of
// calls, what flush() owes, and the out_cap refusal.  Stand-alone, built with -fsanitize=undefined,address by
// tests/test_fft_filter_plan_check.py.
#include "hostlogic/fft_filter_plan.hpp"

#include <cstdio>
#include <limits>
#include <vector>

using namespace gr4pm::hostlogic;
typedef __int128 i128;

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

static const i128 N = 2048;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static FftFilterSizes sizes_128(i128 L, i128 V)
{
    if (L < 1) return FftFilterSizes::no_taps;
    if (L > N - 63) return FftFilterSizes::too_many_taps;
    if (V == 0) return FftFilterSizes::ok; // the default
    if (V > N - 64) return FftFilterSizes::overlap_long;
    if (V < L - 1) return FftFilterSizes::overlap_short;
    return FftFilterSizes::ok;
}

static void check_validation()
{
    bool seen[5] = {};
    for (uint64_t L : {0ull, 1ull, 2ull, 3ull, 64ull, 200ull, 257ull, 1025ull, 1984ull, 1985ull, 1986ull, 4096ull, ~0ull})
        for (uint64_t V : {0ull, 1ull, 2ull, 63ull, 64ull, 199ull, 256ull, 1024ull, 1983ull, 1984ull, 1985ull, 2048ull, ~0ull}) {
            ++cases;
            const FftFilterSizes got = fft_filter_check_sizes(L, V);
            seen[static_cast<int>(got)] = true;
            CHECK(got == sizes_128(L, V), "L %llu V %llu", (unsigned long long)L, (unsigned long long)V);
            if (V <= 1984) { // set_taps() on a handle with this overlap: no default, V itself counts
                const FftFilterSizes again = fft_filter_check_new_taps(L, static_cast<uint32_t>(V));
                const FftFilterSizes want = L < 1 ? FftFilterSizes::no_taps
                                                  : L > 1985 ? FftFilterSizes::too_many_taps
                                                             : static_cast<i128>(V) < static_cast<i128>(L) - 1 ? FftFilterSizes::overlap_short
                                                                                                                 : FftFilterSizes::ok;
                CHECK(again == want, "set_taps L %llu V %llu", (unsigned long long)L, (unsigned long long)V);
            }
        }
    for (int r = 0; r < 5; ++r) CHECK(seen[r], "refusal %d was never given", r);
    for (size_t L = 1; L <= 1985; ++L) {
        ++cases;
        const size_t V = fft_filter_default_overlap(L);
        CHECK(V + 1 >= L && V <= 1984 && (V % 256 == 0 || V == 1984) && (V < 256 || V - 256 + 1 < L), "L %zu V %zu", L, V);
        CHECK(fft_filter_check_sizes(L, V) == FftFilterSizes::ok, "the default overlap of L %zu is refused", L);
    }
    // a non-finite tap
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<float> taps(2 * 7, 0.25f);
    ++cases;
    CHECK(fft_filter_first_bad_tap(taps.data(), 7) == 7, "finite taps");
    CHECK(fft_filter_first_bad_tap(taps.data(), 0) == 0, "no taps");
    for (size_t t = 0; t < 7; ++t)
        for (int part = 0; part < 2; ++part)
            for (float bad : {inf, -inf, nan}) {
                ++cases;
                std::vector<float> v = taps;
                v[2 * t + part] = bad;
                CHECK(fft_filter_first_bad_tap(v.data(), 7) == t, "tap %zu part %d", t, part);
            }
}

// segments complete after `taken` samples, from the definition: s >= 0 with s hop - V + N <= taken
static i128 complete_128(i128 taken, i128 hop) { return taken / hop; }

static void check_calls(uint32_t V, const std::vector<size_t>& calls)
{
    const FftFilterShape g = fft_filter_shape(V);
    const i128 hop = N - V;
    CHECK(g.overlap == V && g.hop == hop, "shape V %u", V);
    uint64_t taken = 0;
    i128 delivered = 0;
    for (size_t n : calls) {
        ++cases;
        CHECK(fft_filter_call_fits(n), "n %zu", n);
        const FftFilterPlan p = fft_filter_plan(g, taken, n);
        const i128 before = complete_128(taken, hop), after = complete_128(static_cast<i128>(taken) + n, hop);
        CHECK(p.n_segments == static_cast<size_t>(after - before), "V %u taken %llu n %zu: segments", V, (unsigned long long)taken, n);
        CHECK(p.samples == static_cast<size_t>((after - before) * hop), "samples");
        CHECK(static_cast<i128>(p.carried) == static_cast<i128>(taken) % hop && p.carried < g.hop, "carried");
        CHECK(static_cast<i128>(p.tail) == V + static_cast<i128>(taken) % hop && p.tail < static_cast<size_t>(N), "tail");
        CHECK(static_cast<i128>(p.carried_new) == (static_cast<i128>(taken) + n) % hop, "carried_new");
        CHECK(p.tail_new == V + p.carried_new && p.tail_new < static_cast<size_t>(N), "tail_new");
        // delivered + pending = taken
        CHECK(delivered + p.samples + p.carried_new == static_cast<i128>(taken) + n, "V %u taken %llu n %zu: delivered + pending", V,
              (unsigned long long)taken, n);
        CHECK(static_cast<i128>(p.first_index) == delivered, "first output index");
        // item v of tail ++ input is the stream's sample taken - tail + v (negative: a zero in front)
        const i128 item0 = static_cast<i128>(taken) - p.tail;
        for (size_t i = 0; i < p.n_segments; ++i) {
            if (i == 64 && p.n_segments > 128) i = p.n_segments - 64; // a long call: its first and last segments
            const i128 s = before + i;
            CHECK(item0 + static_cast<i128>(i) * hop == s * hop - V, "V %u taken %llu n %zu: segment %zu begins at the wrong item", V,
                  (unsigned long long)taken, n, i);
            CHECK(fft_filter_segment_end(g, i) <= p.tail + n, "segment %zu reads beyond tail ++ input", i);
            // its kept samples are out[i hop .. i hop + hop) of the call: the stream's s hop ..
            CHECK(static_cast<i128>(p.first_index) + static_cast<i128>(i) * hop == s * hop, "output position");
        }
        // the new tail is the last tail_new items of tail ++ input
        CHECK(p.tail_new <= p.tail + n, "the new tail reaches in front of tail ++ input");
        // the out_cap refusal: exactly below the samples
        CHECK(!fft_filter_refuses(p, p.samples) && !fft_filter_refuses(p, p.samples + 1), "room is refused");
        CHECK(p.samples == 0 || fft_filter_refuses(p, p.samples - 1), "one too small is not refused");
        delivered += p.samples;
        taken += n;
        // flush() owes exactly what is carried, and the zeros complete one segment
        const FftFilterFlush f = fft_filter_flush(g, taken);
        CHECK(f.owed == p.carried_new, "flush owes %zu, carried %zu", f.owed, p.carried_new);
        CHECK(f.owed ? f.owed + f.zeros == g.hop : f.zeros == 0, "flush zeros");
        if (f.owed) {
            const FftFilterPlan z = fft_filter_plan(g, taken, f.zeros);
            CHECK(z.n_segments == 1 && z.carried_new == 0 && fft_filter_segment_end(g, 0) == z.tail + f.zeros, "the flush segment");
            CHECK(delivered + f.owed == static_cast<i128>(taken), "total out equals total in");
        }
    }
    CHECK(delivered == complete_128(taken, hop) * hop, "V %u: samples in total", V);
}

int main()
{
    check_validation();
    CHECK(!fft_filter_call_fits((size_t(1) << 40) + 1) && fft_filter_call_fits(size_t(1) << 40), "the call's limit");
    for (uint32_t V : {0u, 1u, 63u, 64u, 256u, 1024u, 1983u, 1984u}) {
        const size_t hop = 2048 - V, Nn = 2048;
        const size_t few = hop - 3;
        const std::vector<std::vector<size_t>> seqs = {
            {0, 1, hop - 1, hop, hop + 1, Nn - 1, Nn, Nn + 1, 3 * Nn + 7},
            {3 * Nn + 7, Nn + 1, Nn, Nn - 1, hop + 1, hop, hop - 1, 1, 0},
            {few, 1, 1, 1, 1, few, 1, 1, 1, 1, 1, 5 * hop + 3},
            {size_t(1) << 40, 1, hop, size_t(1) << 33},
        };
        for (const auto& seq : seqs) check_calls(V, seq);
        std::vector<size_t> rnd;
        for (int i = 0; i < 200; ++i) rnd.push_back(static_cast<size_t>(rng() % (i % 7 == 0 ? 9000 : 40)));
        check_calls(V, rnd);
    }
    std::printf("fft_filter_plan_check: %llu cases, %llu failures\n", cases, failures);
    return failures ? 1 : 0;
}
