// Sweeps csrc/hostlogic/fft_duc_plan.hpp (the FftDuc's host side) against restatements in __int128
// from a_s = s hop - V alone: every refusal of the validation (fft_duc_mixed_plan.hpp's, asked with K equal entries, which
// is what an FftDuc's create asks), the shape, and for every I in 4 .. 64 with a set of
// overlaps the segments, carried items, samples and segment positions of sequences of calls.  Stand-alone, built with
// -fsanitize=undefined,address by tests/test_fft_duc_plan_check.py.
#include "hostlogic/fft_duc_mixed_plan.hpp"

#include <cstdio>
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

static i128 floor_div(i128 a, i128 b) // b > 0
{
    i128 q = a / b;
    if (a % b != 0 && a < 0) --q;
    return q;
}
static i128 mod(i128 a, i128 b) { return a - floor_div(a, b) * b; }

static const i128 kTwo64 = static_cast<i128>(1) << 64;
static const i128 N = 2048;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static FftDucMixedRefusal refusal_128(i128 K, i128 I, i128 R, i128 L, i128 V)
{
    auto pow2 = [](i128 v) {
        for (i128 p = 1; p <= 4096; p *= 2)
            if (v == p) return true;
        return false;
    };
    if (K < 1 || K > 64) return FftDucMixedRefusal::channels;
    if (!pow2(I) || I < 4 || I > 64) return FftDucMixedRefusal::interpolation;
    if (!pow2(R) || R > I) return FftDucMixedRefusal::images;
    if (L < 1) return FftDucMixedRefusal::taps;
    if (mod(V, I) != 0) return FftDucMixedRefusal::overlap_multiple;
    if (N - V < 64) return FftDucMixedRefusal::overlap_high;
    if (V < L - 1) return FftDucMixedRefusal::overlap_low;
    return FftDucMixedRefusal::none;
}

static void check_validation()
{
    bool seen[8] = {};
    for (uint64_t K : {0ull, 1ull, 64ull, 65ull})
        for (uint64_t I : {0ull, 1ull, 2ull, 4ull, 12ull, 16ull, 64ull, 128ull})
            for (uint64_t R : {0ull, 1ull, 2ull, 3ull, 16ull, 64ull, 128ull})
                for (uint64_t L : {0ull, 1ull, 2ull, 192ull, 257ull, 1985ull, 1986ull})
                    for (uint64_t V : {0ull, 4ull, 64ull, 100ull, 191ull, 192ull, 256ull, 1984ull, 1985ull, 2048ull, 4096ull}) {
                        ++cases;
                        const std::vector<size_t> Is(K, I), Rs(K, R), Ls(K, L); // K equal rows
                        const FftDucMixedRefusal got = fft_duc_mixed_validate(K, Is.data(), Rs.data(), Ls.data(), V).refusal;
                        seen[static_cast<int>(got)] = true;
                        CHECK(got == refusal_128(K, I, R, L, V), "K %llu I %llu R %llu L %llu V %llu", (unsigned long long)K,
                              (unsigned long long)I, (unsigned long long)R, (unsigned long long)L, (unsigned long long)V);
                    }
    for (int r = 0; r < 8; ++r) CHECK(seen[r], "refusal %d was never given", r);
    for (size_t L : {1, 2, 48, 192, 256, 257, 258, 768, 1985}) {
        ++cases;
        const size_t Ls[3] = {L, L, L};
        const size_t V = fft_duc_mixed_default_overlap(3, Ls);
        CHECK(V % 256 == 0 && V + 1 >= L && (V == 0 || V - 256 + 1 < L), "L %zu V %zu", L, V);
    }
}

// segments complete after `taken` items per row, from the definition: s >= 0 whose last item a_s / I + B - 1 was taken,
// a_s + N <= taken I
static i128 complete_128(i128 taken, i128 hop, i128 V, i128 I)
{
    const i128 room = taken * I - N + V; // s hop <= room
    return room < 0 ? 0 : floor_div(room, hop) + 1;
}

static void check_calls(uint32_t I, uint32_t V, uint64_t start, const std::vector<size_t>& calls)
{
    const FftDucShape g = fft_duc_shape(I, V);
    const i128 hop = N - V, B = N / I;
    CHECK(g.hop == hop && static_cast<i128>(g.hop_items) * I == hop && static_cast<i128>(g.keep) * I == V && g.overlap == V &&
              g.keep + g.hop_items == B,
          "shape I %u V %u", I, V);
    uint64_t taken = 0;
    i128 samples = 0;
    size_t carried = g.keep;
    for (size_t n : calls) {
        ++cases;
        const FftDucPlan p = fft_duc_plan(g, taken, n);
        const i128 before = complete_128(taken, hop, V, I), after = complete_128(static_cast<i128>(taken) + n, hop, V, I);
        CHECK(p.segments_before == static_cast<uint64_t>(before), "I %u V %u taken %llu: before", I, V, (unsigned long long)taken);
        CHECK(p.n_segments == static_cast<size_t>(after - before), "I %u V %u taken %llu n %zu: segments", I, V,
              (unsigned long long)taken, n);
        CHECK(p.samples == static_cast<size_t>((after - before) * hop), "samples");
        CHECK(p.carried == carried && p.carried < static_cast<size_t>(B) && p.left < static_cast<size_t>(B),
              "I %u V %u taken %llu n %zu: carried %zu (%zu) -> %zu", I, V, (unsigned long long)taken, n, p.carried, carried, p.left);
        CHECK(static_cast<i128>(p.carried) == V / I + mod(taken, hop / I), "carried is V / I + taken mod hopI");
        // item v of the call's carried ++ input is the row's item taken - p.carried + v (negative: a zero in front)
        const i128 item0 = static_cast<i128>(taken) - p.carried;
        for (size_t i = 0; i < p.n_segments; ++i) {
            if (i == 64 && p.n_segments > 128) i = p.n_segments - 64; // a long call: its first and last segments
            const i128 s = before + i, a_s = s * hop - V;
            CHECK(mod(a_s, I) == 0, "a_s is no multiple of I");
            CHECK((item0 + static_cast<i128>(i) * g.hop_items) * I == a_s, "I %u V %u taken %llu n %zu: segment %zu begins at the wrong item",
                  I, V, (unsigned long long)taken, n, i);
            CHECK(static_cast<i128>(i) * g.hop_items + B <= static_cast<i128>(p.carried) + n, "segment %zu reads beyond the call", i);
            CHECK((i < p.tail_segments) == (i * g.hop_items < p.carried), "tail_segments");
            const uint64_t idx = fft_duc_item_index(g, start, static_cast<uint64_t>(s));
            CHECK(idx == static_cast<uint64_t>(mod(static_cast<i128>(start) + a_s, kTwo64)), "item_index");
        }
        // what stays: from the first incomplete segment's first item (the zeros in front included) to the end of the row
        const i128 a_next = after * hop - V, end = static_cast<i128>(taken) + n;
        CHECK(static_cast<i128>(p.left) == end - a_next / I && mod(a_next, I) == 0, "I %u V %u taken %llu n %zu: left %zu", I, V,
              (unsigned long long)taken, n, p.left);
        samples += p.samples;
        taken += n;
        carried = p.left;
    }
    // the samples of all calls: hop for every segment that is complete after all of them
    CHECK(samples == complete_128(taken, hop, V, I) * hop, "I %u V %u: samples in total", I, V);
}

int main()
{
    check_validation();
    for (uint32_t I : {4u, 8u, 16u, 32u, 64u}) {
        const std::vector<uint32_t> Vs = {0u, I, 64u, 256u, 512u, 1024u, 1984u - I, 1984u};
        for (uint32_t V : Vs) {
            if (V % I || V > 1984) {
                std::printf("overlap %u does not fit I = %u\n", V, I);
                return 1;
            }
            const size_t hopI = (2048 - V) / I, B = 2048 / I;
            const size_t few = hopI > 3 ? hopI - 3 : 0;
            const std::vector<std::vector<size_t>> seqs = {
                {0, 1, hopI - 1, hopI, hopI + 1, B - 1, B, B + 1, 3 * B + 7},
                {3 * B + 7, B + 1, B, B - 1, hopI + 1, hopI, hopI - 1, 1, 0},
                {few, 1, 1, 1, 1, few, 1, 1, 1, 1, 1, 5 * hopI + 3},
                {size_t(1) << 40, 1, hopI, size_t(1) << 33},
            };
            for (const auto& seq : seqs)
                for (uint64_t start : {0ull, (1ull << 40) + 3, ~0ull}) check_calls(I, V, start, seq);
            std::vector<size_t> rnd;
            for (int i = 0; i < 200; ++i) rnd.push_back(static_cast<size_t>(rng() % (i % 7 == 0 ? 9000 : 40)));
            check_calls(I, V, 12345, rnd);
        }
    }
    std::printf("fft_duc_plan_check: %llu cases, %llu failures\n", cases, failures);
    return failures ? 1 : 0;
}
