// Sweeps csrc/hostlogic/fft_ddc_plan.hpp (the FftDdc's host side) against restatements in __int128:
// the nearest bin, the rotator's phase and the table's word, the validation (fft_ddc_mixed_plan.hpp's, asked with K equal
// entries, which is what an FftDdc's create asks), and for every D in 4 .. 64 with a set of overlaps the segments, tails
// and frames of sequences of calls.  Stand-alone, built with -fsanitize=undefined,address by
// tests/test_fft_ddc_plan_check.py.
#include "hostlogic/fft_ddc_mixed_plan.hpp"

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

static const i128 kOne = static_cast<i128>(1) << 32;
static const i128 N = 2048;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static void check_words()
{
    std::vector<uint32_t> ws = {0u, 1u, (1u << 20) - 1, 1u << 20, (1u << 20) + 1, (1u << 21) - 1, 1u << 21, 3u << 20, 0x7FFFFFFFu,
                                0x80000000u, 0xFFEFFFFFu, 0xFFF00000u, 0xFFFFFFFFu};
    for (int r = 0; r < 2000; ++r) ws.push_back(static_cast<uint32_t>(rng()));
    for (uint32_t w : ws) {
        ++cases;
        // floor(w N / 2^32 + 1 / 2) mod N
        const i128 c = mod(floor_div(2 * static_cast<i128>(w) * N + kOne, 2 * kOne), N);
        CHECK(fft_ddc_bin(w) == static_cast<uint32_t>(c), "w %u", w);
        for (int r = 0; r < 8; ++r) {
            const uint64_t i = r == 0 ? 0 : r == 1 ? ~0ull : rng();
            const uint32_t p = static_cast<uint32_t>(rng() % 2048);
            const i128 phi = mod(static_cast<i128>(w) * static_cast<i128>(i) - c * (kOne / N) * p, kOne);
            CHECK(fft_ddc_phi(w, static_cast<uint32_t>(c), i, p) == static_cast<uint32_t>(phi), "w %u i %llu p %u", w,
                  static_cast<unsigned long long>(i), p);
            const int32_t u = static_cast<int32_t>(rng() % 2048) - 1024;
            const i128 psi = mod((c + u) * (kOne / N) - static_cast<i128>(w), kOne);
            CHECK(fft_ddc_table_word(w, static_cast<uint32_t>(c), u) == static_cast<uint32_t>(psi), "w %u u %d", w, u);
        }
    }
}

static void check_validation()
{
    for (uint64_t K : {0ull, 1ull, 64ull, 65ull})
        for (uint64_t D : {0ull, 1ull, 2ull, 4ull, 12ull, 16ull, 64ull, 128ull})
            for (uint64_t R : {0ull, 1ull, 2ull, 3ull, 16ull, 64ull, 128ull})
                for (uint64_t L : {0ull, 1ull, 2ull, 192ull, 257ull, 1985ull, 1986ull})
                    for (uint64_t V : {0ull, 4ull, 64ull, 100ull, 191ull, 192ull, 256ull, 1984ull, 1985ull, 2048ull, 4096ull}) {
                        ++cases;
                        const bool pow2D = D == 4 || D == 16 || D == 64;
                        const bool okR = (R == 1 || R == 2 || R == 16 || R == 64) && R <= D;
                        const bool ok = K >= 1 && K <= 64 && pow2D && okR && L >= 1 && V % (D ? D : 1) == 0 &&
                                        static_cast<i128>(V) >= static_cast<i128>(L) - 1 && V <= 2048 - 64;
                        const std::vector<size_t> Ds(K, D), Rs(K, R), Ls(K, L); // K equal channels
                        CHECK((fft_ddc_mixed_validate(K, Ds.data(), Rs.data(), Ls.data(), V).refusal == FftDdcMixedRefusal::none) == ok,
                              "K %llu D %llu R %llu L %llu V %llu",
                              (unsigned long long)K, (unsigned long long)D, (unsigned long long)R, (unsigned long long)L,
                              (unsigned long long)V);
                    }
    for (size_t L : {1, 2, 48, 192, 256, 257, 258, 768, 1985}) {
        ++cases;
        const size_t Ds[3] = {16, 16, 16}, Ls[3] = {L, L, L};
        const size_t V = fft_ddc_mixed_default_overlap(3, Ds, Ls);
        CHECK(V % 256 == 0 && V + 1 >= L && (V == 0 || V - 256 + 1 < L), "L %zu V %zu", L, V);
    }
}

// segments complete after `taken` samples, from the definition: s >= 0 with a_s + N <= taken
static i128 complete_128(i128 taken, i128 hop, i128 V, i128 D)
{
    const i128 room = taken - N + V - D + 1; // s hop <= room
    return room < 0 ? 0 : floor_div(room, hop) + 1;
}

static void check_calls(uint32_t D, uint32_t V, uint64_t start, const std::vector<size_t>& calls)
{
    const FftDdcShape g = fft_ddc_shape(D, V);
    const i128 hop = N - V;
    CHECK(g.hop == hop && g.frames * D == g.hop && g.first * D == V, "shape D %u V %u", D, V);
    uint64_t taken = 0;
    i128 frames = 0;
    size_t tail = g.zeros;
    for (size_t n : calls) {
        ++cases;
        const FftDdcPlan p = fft_ddc_plan(g, taken, n);
        const i128 before = complete_128(taken, hop, V, D), after = complete_128(static_cast<i128>(taken) + n, hop, V, D);
        CHECK(p.segments_before == static_cast<uint64_t>(before), "D %u V %u taken %llu: before", D, V, (unsigned long long)taken);
        CHECK(p.n_segments == static_cast<size_t>(after - before), "D %u V %u taken %llu n %zu: segments", D, V,
              (unsigned long long)taken, n);
        CHECK(p.frames == static_cast<size_t>((after - before) * (hop / D)), "frames");
        CHECK(p.drop + p.n_used == n && p.tail == tail && p.tail < 2048 && p.tail_new < 2048, "D %u V %u taken %llu n %zu: tail %zu (%zu) -> %zu",
              D, V, (unsigned long long)taken, n, p.tail, tail, p.tail_new);
        // the call's virtual item v is the stream's item taken + p.drop - p.tail + v (negative: a zero in front)
        const i128 item0 = static_cast<i128>(taken) + p.drop - p.tail;
        for (size_t i = 0; i < p.n_segments; ++i) {
            if (i == 64 && p.n_segments > 128) i = p.n_segments - 64; // a long call: its first and last segments
            const i128 s = before + i, a_s = s * hop - V + D - 1;
            CHECK(item0 + static_cast<i128>(i) * hop == a_s, "D %u V %u taken %llu n %zu: segment %zu begins at the wrong item", D, V,
                  (unsigned long long)taken, n, i);
            CHECK(i * g.hop + 2048 <= p.tail + p.n_used, "segment %zu reads beyond the call", i);
            CHECK((i < p.tail_segments) == (i * g.hop < p.tail), "tail_segments");
            const uint64_t idx = fft_ddc_segment_index(g, start, static_cast<uint64_t>(s));
            CHECK(idx == static_cast<uint64_t>(mod(static_cast<i128>(start) + a_s, kOne * kOne)), "segment_index");
        }
        // what stays: from the first incomplete segment's begin (the zeros in front included) to the end of the stream
        const i128 a_next = after * hop - V + D - 1, end = static_cast<i128>(taken) + n;
        CHECK(static_cast<i128>(p.tail_new) == (end > a_next ? end - a_next : 0), "D %u V %u taken %llu n %zu: tail_new %zu", D, V,
              (unsigned long long)taken, n, p.tail_new);
        frames += p.frames;
        taken += n;
        tail = p.tail_new;
    }
    // the frames of all calls: hop / D for every segment that is complete after all of them
    CHECK(frames == complete_128(taken, hop, V, D) * (hop / D), "D %u V %u: frames in total", D, V);
}

int main()
{
    check_words();
    check_validation();
    for (uint32_t D : {4u, 8u, 16u, 32u, 64u}) {
        std::vector<uint32_t> Vs = {0u, D, 64u, 256u, 512u, 1024u, 1984u - D, 1984u};
        for (uint32_t V : Vs) {
            if (V % D || V > 1984) continue;
            const size_t hop = 2048 - V;
            const std::vector<std::vector<size_t>> seqs = {
                {0, 1, hop - 1, hop, 2047, 2048, 2049, 3 * 2048 + 7},
                {3 * 2048 + 7, 2049, 2048, 2047, hop, hop - 1, 1, 0},
                {1, 1, 1, D - 2, 1, 1, 1, V + 1, 1, 1, hop - 3, 1, 1, 1, 1, 5 * hop + 77},
                {size_t(1) << 40, 1, hop, size_t(1) << 33},
            };
            for (const auto& seq : seqs)
                for (uint64_t start : {0ull, (1ull << 40) + 3, ~0ull}) check_calls(D, V, start, seq);
            std::vector<size_t> rnd;
            for (int i = 0; i < 200; ++i) rnd.push_back(static_cast<size_t>(rng() % (i % 7 == 0 ? 9000 : 40)));
            check_calls(D, V, 12345, rnd);
        }
    }
    std::printf("fft_ddc_plan_check: %llu cases, %llu failures\n", cases, failures);
    return failures ? 1 : 0;
}
