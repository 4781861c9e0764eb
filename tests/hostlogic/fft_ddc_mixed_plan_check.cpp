// Sweeps csrc/hostlogic/fft_ddc_mixed_plan.hpp (the MixedFftDdc's host side) against restatements in
// __int128 from a_s = s hop - V + Dmax - 1 and the frame grid i = n D_k + D_k - 1 alone: every refusal of the validation,
// the default overlap, and for all 31 non-empty subsets of {4, 8, 16, 32, 64} as the decimations of a handle, with several
// overlaps and start indices, the kept items of every channel and the segments, tails and per-channel frames of the call
// sequences of fft_ddc_plan_check.cpp.  Stand-alone, built with -fsanitize=undefined,address by
// tests/test_fft_ddc_mixed_plan_check.py.
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

static bool pow2(i128 v) { return v > 0 && (v & (v - 1)) == 0; }

// the definition's conditions, in the order the header documents for the refusals
static FftDdcMixedRefusal expect(const std::vector<size_t>& D, const std::vector<size_t>& R, const std::vector<size_t>& L, size_t V,
                                 size_t& channel)
{
    const size_t K = D.size();
    channel = 0;
    if (K < 1 || K > 64) return FftDdcMixedRefusal::channels;
    for (size_t k = 0; k < K; ++k)
        if (!pow2(D[k]) || D[k] < 4 || D[k] > 64) return channel = k, FftDdcMixedRefusal::decimation;
    for (size_t k = 0; k < K; ++k)
        if (!pow2(R[k]) || R[k] > D[k]) return channel = k, FftDdcMixedRefusal::images;
    for (size_t k = 0; k < K; ++k)
        if (L[k] < 1) return channel = k, FftDdcMixedRefusal::taps;
    i128 Dmax = 0;
    for (size_t d : D) Dmax = static_cast<i128>(d) > Dmax ? static_cast<i128>(d) : Dmax;
    if (static_cast<i128>(V) % Dmax) return FftDdcMixedRefusal::overlap_multiple;
    if (static_cast<i128>(V) > N - 64) return FftDdcMixedRefusal::overlap_high;
    for (size_t k = 0; k < K; ++k)
        if (static_cast<i128>(V) - (Dmax - static_cast<i128>(D[k])) < static_cast<i128>(L[k]) - 1) return channel = k, FftDdcMixedRefusal::overlap_low;
    return FftDdcMixedRefusal::none;
}

static void check_one_validation(const std::vector<size_t>& D, const std::vector<size_t>& R, const std::vector<size_t>& L, size_t V)
{
    ++cases;
    size_t channel = 0;
    const FftDdcMixedRefusal want = expect(D, R, L, V, channel);
    const FftDdcMixedVerdict got = fft_ddc_mixed_validate(D.size(), D.data(), R.data(), L.data(), V);
    CHECK(got.refusal == want && got.channel == channel, "K %zu D0 %zu R0 %zu L0 %zu V %zu: refusal %d (channel %zu), expected %d (%zu)",
          D.size(), D.empty() ? 0 : D[0], R.empty() ? 0 : R[0], L.empty() ? 0 : L[0], V, static_cast<int>(got.refusal), got.channel,
          static_cast<int>(want), channel);
}

static void check_validation()
{
    // the number of channels
    for (size_t K : {0, 1, 2, 64, 65}) check_one_validation(std::vector<size_t>(K, 16), std::vector<size_t>(K, 2), std::vector<size_t>(K, 192), 256);
    // one channel beside a good one (D 64, R 2, L 100), in both positions: every refusal of a channel's own sizes and of
    // the overlap, the new condition among them (L - 1 <= V < Dmax - D_k + L - 1)
    for (size_t D : {0, 1, 2, 3, 4, 8, 12, 16, 32, 64, 128})
        for (size_t R : {0, 1, 2, 3, 4, 16, 64, 128})
            for (size_t L : {0, 1, 2, 192, 193, 197, 253, 257, 720, 765, 1985, 1986})
                for (size_t V : {0, 64, 100, 128, 192, 256, 704, 768, 832, 1920, 1984, 2048, 4096})
                    for (int order = 0; order < 2; ++order) {
                        std::vector<size_t> Ds = {D, 64}, Rs = {R, 2}, Ls = {L, 100};
                        if (order) Ds = {64, D}, Rs = {2, R}, Ls = {100, L};
                        check_one_validation(Ds, Rs, Ls, V);
                    }
    // the issue's case: L_0 - 1 <= V, but Dmax - D_0 + L_0 - 1 > V
    {
        ++cases;
        const size_t D[2] = {4, 64}, R[2] = {2, 2}, L[2] = {720, 100};
        const FftDdcMixedVerdict v = fft_ddc_mixed_validate(2, D, R, L, 768);
        CHECK(v.refusal == FftDdcMixedRefusal::overlap_low && v.channel == 0, "D (4, 64) L_0 720 V 768");
        const size_t L2[2] = {709, 100}; // 60 + 708 = 768
        CHECK(fft_ddc_mixed_validate(2, D, R, L2, 768).refusal == FftDdcMixedRefusal::none, "D (4, 64) L_0 709 V 768");
        CHECK(fft_ddc_mixed_default_overlap(2, D, L) == 1024 && fft_ddc_mixed_default_overlap(2, D, L2) == 768, "default overlap");
    }
    // V = 0: equal decimations and one tap only
    for (size_t Da : {4, 64})
        for (size_t Db : {4, 64})
            for (size_t La : {1, 2})
                check_one_validation({Da, Db}, {1, 1}, {La, 1}, 0);
    // the default overlap: the smallest multiple of 256 that the overlap_low condition accepts for every channel
    for (int r = 0; r < 2000; ++r) {
        ++cases;
        const size_t K = 1 + rng() % 6;
        std::vector<size_t> D(K), R(K, 1), L(K);
        for (size_t k = 0; k < K; ++k) D[k] = size_t(4) << (rng() % 5), L[k] = 1 + rng() % 1900;
        const size_t V = fft_ddc_mixed_default_overlap(K, D.data(), L.data());
        size_t channel;
        CHECK(V % 256 == 0, "default overlap %zu", V);
        if (V <= 1984) {
            CHECK(expect(D, R, L, V, channel) == FftDdcMixedRefusal::none, "default overlap %zu is refused", V);
            CHECK(V == 0 || expect(D, R, L, V - 256, channel) == FftDdcMixedRefusal::overlap_low, "default overlap %zu is not the smallest", V);
        } else {
            CHECK(expect(D, R, L, V, channel) == FftDdcMixedRefusal::overlap_high, "default overlap %zu", V);
        }
    }
}

// segments complete after `taken` samples, from the definition: s >= 0 with a_s + N <= taken
static i128 complete_128(i128 taken, i128 hop, i128 V, i128 Dmax)
{
    const i128 room = taken - N + V - Dmax + 1; // s hop <= room
    return room < 0 ? 0 : floor_div(room, hop) + 1;
}

// the kept items of every channel, from a_s and the frame grid
static void check_channels(const std::vector<size_t>& D, const std::vector<size_t>& R, uint32_t Dmax, uint32_t V)
{
    const i128 hop = N - V;
    std::vector<size_t> offsets(D.size());
    const size_t total = fft_ddc_mixed_table_offsets(D.size(), D.data(), R.data(), offsets.data());
    i128 at = 0;
    for (size_t k = 0; k < D.size(); ++k) {
        ++cases;
        const i128 Dk = static_cast<i128>(D[k]), Bk = N / Dk;
        const FftDdcMixedChannel c = fft_ddc_mixed_channel(Dmax, V, static_cast<uint32_t>(D[k]));
        CHECK(c.frames * Dk == hop, "D %zu V %u: frames", D[k], V);
        // n' = first_k is the first whose frame is not negative in segment 0, and frame 0 it is: a_0 + n' D_k = D_k - 1
        CHECK(-static_cast<i128>(V) + Dmax - 1 + c.first * Dk == Dk - 1, "D %zu Dmax %u V %u: first %u", D[k], Dmax, V, c.first);
        CHECK(c.first * Dk == static_cast<i128>(V) - Dmax + Dk, "smallest kept item");
        CHECK((c.first + c.frames - 1) * Dk == N - Dmax && c.first + c.frames <= Bk, "D %zu Dmax %u V %u: largest kept item", D[k], Dmax, V);
        for (i128 s : {static_cast<i128>(0), static_cast<i128>(1), static_cast<i128>(149795), static_cast<i128>(1) << 40})
            for (uint32_t f : {0u, 1u, c.frames / 2, c.frames - 1}) {
                const i128 a_s = s * hop - V + Dmax - 1, n = s * c.frames + f;
                CHECK(a_s + (c.first + f) * Dk == n * Dk + Dk - 1, "D %zu Dmax %u V %u: frame %u of a segment is off the Ddc's grid", D[k], Dmax, V, f);
            }
        CHECK(static_cast<i128>(offsets[k]) == at, "table offset of channel %zu", k);
        at += static_cast<i128>(R[k]) * Bk;
    }
    CHECK(static_cast<i128>(total) == at, "table size");
}

static void check_calls(const std::vector<size_t>& D, uint32_t Dmax, uint32_t V, uint64_t start, const std::vector<size_t>& calls)
{
    const FftDdcShape g = fft_ddc_shape(Dmax, V);
    const i128 hop = N - V;
    uint64_t taken = 0;
    std::vector<i128> frames(D.size(), 0);
    size_t tail = g.zeros;
    for (size_t n : calls) {
        ++cases;
        const FftDdcPlan p = fft_ddc_plan(g, taken, n);
        const i128 before = complete_128(taken, hop, V, Dmax), after = complete_128(static_cast<i128>(taken) + n, hop, V, Dmax);
        CHECK(p.segments_before == static_cast<uint64_t>(before) && p.n_segments == static_cast<size_t>(after - before),
              "Dmax %u V %u taken %llu n %zu: segments", Dmax, V, (unsigned long long)taken, n);
        CHECK(p.drop + p.n_used == n && p.tail == tail && p.tail < 2048 && p.tail_new < 2048, "Dmax %u V %u taken %llu n %zu: tail", Dmax, V,
              (unsigned long long)taken, n);
        const i128 item0 = static_cast<i128>(taken) + p.drop - p.tail;
        for (size_t i = 0; i < p.n_segments; ++i) {
            if (i == 16 && p.n_segments > 32) i = p.n_segments - 16; // a long call: its first and last segments
            const i128 s = before + i, a_s = s * hop - V + Dmax - 1;
            CHECK(item0 + static_cast<i128>(i) * hop == a_s, "Dmax %u V %u taken %llu n %zu: segment %zu begins at the wrong item", Dmax, V,
                  (unsigned long long)taken, n, i);
            CHECK(i * g.hop + 2048 <= p.tail + p.n_used, "segment %zu reads beyond the call", i);
            CHECK(fft_ddc_segment_index(g, start, static_cast<uint64_t>(s)) == static_cast<uint64_t>(mod(static_cast<i128>(start) + a_s, kTwo64)),
                  "segment_index");
        }
        for (size_t k = 0; k < D.size(); ++k) {
            const FftDdcMixedChannel c = fft_ddc_mixed_channel(Dmax, V, static_cast<uint32_t>(D[k]));
            const size_t f = fft_ddc_mixed_frames(p, c);
            // the frames n of the Ddc's grid at D_k whose segment is complete: those of [before, after)
            CHECK(static_cast<i128>(f) == (after - before) * (hop / static_cast<i128>(D[k])), "frames of channel %zu", k);
            // the call's first frame continues the row: before hop / D_k, whose newest sample is a_before + first_k D_k
            const i128 n0 = frames[k];
            CHECK(n0 == before * c.frames && n0 * D[k] + D[k] - 1 == before * hop - V + Dmax - 1 + static_cast<i128>(c.first) * D[k],
                  "channel %zu: the call's first frame", k);
            frames[k] += f;
        }
        taken += n;
        tail = p.tail_new;
    }
    for (size_t k = 0; k < D.size(); ++k)
        CHECK(frames[k] == complete_128(taken, hop, V, Dmax) * (hop / static_cast<i128>(D[k])), "Dmax %u V %u: frames of channel %zu in total", Dmax, V, k);
}

int main()
{
    check_validation();
    const size_t all[5] = {4, 8, 16, 32, 64};
    for (unsigned subset = 1; subset < 32; ++subset) {
        std::vector<size_t> D, R;
        for (int b = 4; b >= 0; --b) // any order: here descending, and one decimation twice
            if (subset >> b & 1) D.push_back(all[b]);
        D.push_back(D.back());
        for (size_t d : D) R.push_back(d > 4 && subset % 2 ? d / 2 : 2);
        const uint32_t Dmax = static_cast<uint32_t>(fft_ddc_mixed_max_decimation(D.size(), D.data()));
        const uint32_t Dmin = static_cast<uint32_t>(D[D.size() - 1]);
        for (uint32_t V : {0u, Dmax, 64u, 256u, 512u, 768u, 1024u, 1984u - Dmax, 1984u}) {
            if (V % Dmax || V > 1984 || V < Dmax - Dmin) continue;
            std::vector<size_t> L;
            for (size_t d : D) L.push_back(V - (Dmax - d) + 1); // the longest prototype the overlap takes
            ++cases;
            CHECK(fft_ddc_mixed_validate(D.size(), D.data(), R.data(), L.data(), V).refusal == FftDdcMixedRefusal::none, "subset %u V %u", subset, V);
            L[D.size() - 1] += 1;
            CHECK(fft_ddc_mixed_validate(D.size(), D.data(), R.data(), L.data(), V).refusal == FftDdcMixedRefusal::overlap_low, "subset %u V %u", subset, V);
            check_channels(D, R, Dmax, V);
            const size_t hop = 2048 - V;
            const std::vector<std::vector<size_t>> seqs = {
                {0, 1, hop - 1, hop, 2047, 2048, 2049, 3 * 2048 + 7},
                {3 * 2048 + 7, 2049, 2048, 2047, hop, hop - 1, 1, 0},
                {1, 1, 1, Dmax - 2, 1, 1, 1, V + 1, 1, 1, hop - 3, 1, 1, 1, 1, 5 * hop + 77},
                {size_t(1) << 40, 1, hop, size_t(1) << 33},
            };
            for (const auto& seq : seqs)
                for (uint64_t start : {0ull, (1ull << 40) + 3, ~0ull}) check_calls(D, Dmax, V, start, seq);
            std::vector<size_t> rnd;
            for (int i = 0; i < 200; ++i) rnd.push_back(static_cast<size_t>(rng() % (i % 7 == 0 ? 9000 : 40)));
            check_calls(D, Dmax, V, 12345, rnd);
        }
    }
    std::printf("fft_ddc_mixed_plan_check: %llu cases, %llu failures\n", cases, failures);
    return failures ? 1 : 0;
}
