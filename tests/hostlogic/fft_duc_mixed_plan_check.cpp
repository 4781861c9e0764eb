// Sweeps csrc/hostlogic/fft_duc_mixed_plan.hpp (the MixedFftDuc's host side) against restatements in
// __int128 from a_s = s hop - V and "item m of row k sits at output sample m I_k" alone: every refusal of the validation,
// the default overlap, the table and carried-item offsets, and for all 31 non-empty subsets of {4, 8, 16, 32, 64} as the
// rows' interpolations with a set of overlaps the segments, the items taken, carried and left per row, the samples and the
// segment positions of sequences of calls counted in slots.  Stand-alone, built with -fsanitize=undefined,address by
// tests/test_fft_duc_mixed_plan_check.py.
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

static bool pow2_128(i128 v)
{
    for (i128 p = 1; p <= 4096; p *= 2)
        if (v == p) return true;
    return false;
}

static FftDucMixedVerdict refusal_128(const std::vector<size_t>& I, const std::vector<size_t>& R, const std::vector<size_t>& L, i128 V)
{
    const size_t K = I.size();
    if (K < 1 || K > 64) return {FftDucMixedRefusal::channels, 0};
    for (size_t k = 0; k < K; ++k)
        if (!pow2_128(I[k]) || I[k] < 4 || I[k] > 64) return {FftDucMixedRefusal::interpolation, k};
    for (size_t k = 0; k < K; ++k)
        if (!pow2_128(R[k]) || R[k] > I[k]) return {FftDucMixedRefusal::images, k};
    for (size_t k = 0; k < K; ++k)
        if (L[k] < 1) return {FftDucMixedRefusal::taps, k};
    i128 Imax = 0;
    for (size_t k = 0; k < K; ++k) Imax = static_cast<i128>(I[k]) > Imax ? static_cast<i128>(I[k]) : Imax;
    if (mod(V, Imax) != 0) return {FftDucMixedRefusal::overlap_multiple, 0};
    if (N - V < 64) return {FftDucMixedRefusal::overlap_high, 0};
    for (size_t k = 0; k < K; ++k)
        if (V < static_cast<i128>(L[k]) - 1) return {FftDucMixedRefusal::overlap_low, k};
    return {FftDucMixedRefusal::none, 0};
}

static void check_validation()
{
    bool seen[8] = {};
    // rows 0 .. K - 2 are plain (I = 16, R = 2, L = L_first); the last row takes the values under test
    for (size_t K : {0, 1, 3, 64, 65})
        for (size_t I_last : {0, 2, 4, 12, 64, 128})
            for (size_t R_last : {0, 1, 2, 3, 64, 128})
                for (size_t L_last : {0, 1, 192, 257, 1986})
                    for (size_t L_first : {1, 600})
                        for (size_t V : {0, 4, 64, 100, 192, 256, 640, 1984, 1985, 2048, 4096}) {
                            ++cases;
                            std::vector<size_t> I(K, 16), R(K, 2), L(K, L_first);
                            if (K) I[K - 1] = I_last, R[K - 1] = R_last, L[K - 1] = L_last;
                            const FftDucMixedVerdict got = fft_duc_mixed_validate(K, I.data(), R.data(), L.data(), V);
                            const FftDucMixedVerdict want = refusal_128(I, R, L, V);
                            seen[static_cast<int>(got.refusal)] = true;
                            CHECK(got.refusal == want.refusal && got.channel == want.channel,
                                  "K %zu I %zu R %zu L %zu / %zu V %zu: %d at %zu, not %d at %zu", K, I_last, R_last, L_last, L_first, V,
                                  static_cast<int>(got.refusal), got.channel, static_cast<int>(want.refusal), want.channel);
                        }
    for (int r = 0; r < 8; ++r) CHECK(seen[r], "refusal %d was never given", r);
    { // the overlap is too low for one row only: 1000 taps on the I = 4 row beside an I = 64 row, V = 768
        ++cases;
        const size_t I[2] = {4, 64}, R[2] = {2, 2}, L[2] = {1000, 768};
        const FftDucMixedVerdict got = fft_duc_mixed_validate(2, I, R, L, 768);
        CHECK(got.refusal == FftDucMixedRefusal::overlap_low && got.channel == 0, "row-specific overlap_low");
        CHECK(fft_duc_mixed_validate(2, I, R, L, 1024).refusal == FftDucMixedRefusal::none, "V = 1024 takes both rows");
        CHECK(fft_duc_mixed_default_overlap(2, L) == 1024, "default overlap of (1000, 768) taps");
    }
    for (size_t La : {1, 2, 48, 192, 256, 257, 258, 768, 1985})
        for (size_t Lb : {1, 257, 1985}) {
            ++cases;
            const size_t L[2] = {La, Lb};
            const size_t V = fft_duc_mixed_default_overlap(2, L), reach = (La > Lb ? La : Lb) - 1;
            CHECK(V % 256 == 0 && V >= reach && (V == 0 || V - 256 < reach), "L %zu %zu V %zu", La, Lb, V);
        }
}

// segments complete after T output samples' worth of items on every row, from the definition: s >= 0 with a_s + N <= T
static i128 complete_128(i128 T, i128 hop, i128 V)
{
    const i128 room = T - N + V; // s hop <= room
    return room < 0 ? 0 : floor_div(room, hop) + 1;
}

static void check_calls(const std::vector<size_t>& I, uint32_t V, uint64_t start, const std::vector<size_t>& calls)
{
    const size_t K = I.size();
    const uint32_t Imax = static_cast<uint32_t>(fft_duc_mixed_max_interpolation(K, I.data()));
    const FftDucShape g = fft_duc_shape(Imax, V);
    const i128 hop = N - V;
    std::vector<FftDucMixedRow> rows(K);
    std::vector<size_t> g_off(K), h_off(K), R(K);
    for (size_t k = 0; k < K; ++k) R[k] = k % 2 ? I[k] : 2;
    const size_t g_total = fft_duc_mixed_table_offsets(K, I.data(), R.data(), g_off.data());
    const size_t h_total = fft_duc_mixed_carried_offsets(K, I.data(), h_off.data());
    uint32_t max_ratio = 1;
    for (size_t k = 0; k < K; ++k) {
        const i128 Ik = I[k], B = N / Ik;
        rows[k] = fft_duc_mixed_row(Imax, V, static_cast<uint32_t>(I[k]));
        CHECK(rows[k].ratio * Ik == Imax && rows[k].hop_items * Ik == hop && rows[k].keep * Ik == V &&
                  rows[k].keep + rows[k].hop_items == B,
              "row %zu of I %zu V %u", k, I[k], V);
        const size_t g_end = k + 1 < K ? g_off[k + 1] : g_total, h_end = k + 1 < K ? h_off[k + 1] : h_total;
        CHECK(g_end - g_off[k] == R[k] * static_cast<size_t>(B), "table offsets of row %zu", k);
        CHECK(h_end - h_off[k] + 1 == static_cast<size_t>(B), "carried offsets of row %zu: room for B - 1 items", k);
        max_ratio = rows[k].ratio > max_ratio ? rows[k].ratio : max_ratio;
    }
    CHECK(fft_duc_mixed_slots_fit((size_t(1) << 40) / max_ratio, max_ratio) && !fft_duc_mixed_slots_fit((size_t(1) << 40) / max_ratio + 1, max_ratio),
          "2^40 items in the longest row");
    uint64_t taken = 0; // slots
    i128 samples = 0;
    std::vector<i128> taken_k(K, 0);
    std::vector<size_t> carried_k(K);
    for (size_t k = 0; k < K; ++k) carried_k[k] = rows[k].keep;
    for (size_t u : calls) {
        ++cases;
        CHECK(fft_duc_mixed_slots_fit(u, max_ratio), "a call of the sweep is refused");
        const FftDucPlan p = fft_duc_plan(g, taken, u);
        const i128 T0 = static_cast<i128>(taken) * Imax, T1 = (static_cast<i128>(taken) + u) * Imax;
        const i128 before = complete_128(T0, hop, V), after = complete_128(T1, hop, V);
        CHECK(p.segments_before == static_cast<uint64_t>(before) && p.n_segments == static_cast<size_t>(after - before),
              "Imax %u V %u taken %llu u %zu: segments", Imax, V, (unsigned long long)taken, u);
        CHECK(p.samples == static_cast<size_t>((after - before) * hop), "samples");
        const i128 pending = mod(taken, hop / Imax);
        for (size_t k = 0; k < K; ++k) {
            const i128 Ik = I[k], B = N / Ik;
            const size_t n = fft_duc_mixed_items(rows[k], u), H = fft_duc_mixed_carried(p, rows[k]), left = fft_duc_mixed_left(p, rows[k]);
            CHECK(static_cast<i128>(n) * Ik == static_cast<i128>(u) * Imax, "row %zu: the items of %zu slots", k, u);
            CHECK(H == carried_k[k] && static_cast<i128>(H) < B && static_cast<i128>(left) < B, "row %zu: carried %zu (%zu) -> %zu", k, H,
                  carried_k[k], left);
            CHECK(static_cast<i128>(H) * Ik == V + pending * Imax, "H_k is (V + pending Imax) / I_k");
            // item v of the row's carried ++ input is its item taken_k - H + v (negative: a zero in front)
            const i128 item0 = taken_k[k] - H;
            for (size_t i = 0; i < p.n_segments; ++i) {
                if (i == 16 && p.n_segments > 32) i = p.n_segments - 16; // a long call: its first and last segments
                const i128 s = before + i, a_s = s * hop - V;
                CHECK(mod(a_s, Ik) == 0, "a_s is no multiple of I_k");
                CHECK((item0 + static_cast<i128>(i) * rows[k].hop_items) * Ik == a_s, "row %zu taken %llu u %zu: segment %zu begins at the wrong item",
                      k, (unsigned long long)taken, u, i);
                CHECK(static_cast<i128>(i) * rows[k].hop_items + B <= static_cast<i128>(H) + n, "row %zu: segment %zu reads beyond the call", k, i);
                if (k == 0) {
                    const uint64_t idx = fft_duc_item_index(g, start, static_cast<uint64_t>(s));
                    CHECK(idx == static_cast<uint64_t>(mod(static_cast<i128>(start) + a_s, kTwo64)), "item_index");
                }
            }
            // what stays: from the first incomplete segment's first item (the zeros in front included) to the row's end
            const i128 a_next = after * hop - V, end = taken_k[k] + n;
            CHECK(static_cast<i128>(left) == end - a_next / Ik && mod(a_next, Ik) == 0, "row %zu taken %llu u %zu: left %zu", k,
                  (unsigned long long)taken, u, left);
            // items taken = items in delivered segments + carried items (of which V / I_k stand for the zeros in front)
            CHECK(end == after * rows[k].hop_items + static_cast<i128>(left) - rows[k].keep, "row %zu: taken = delivered + carried", k);
            taken_k[k] = end;
            carried_k[k] = left;
        }
        samples += p.samples;
        taken += u;
    }
    CHECK(samples == complete_128(static_cast<i128>(taken) * Imax, hop, V) * hop, "Imax %u V %u: samples in total", Imax, V);
}

int main()
{
    check_validation();
    const size_t all[5] = {4, 8, 16, 32, 64};
    for (unsigned set = 1; set < 32; ++set) {
        std::vector<size_t> I;
        for (int b = 4; b >= 0; --b) // the largest first in one half of the subsets, the smallest first in the other
            if (set >> (set % 2 ? b : 4 - b) & 1) I.push_back(all[set % 2 ? b : 4 - b]);
        const uint32_t Imax = static_cast<uint32_t>(fft_duc_mixed_max_interpolation(I.size(), I.data()));
        const std::vector<uint32_t> Vs = {0u, Imax, 256u, 512u, 1024u, 1984u - Imax, 1984u};
        for (uint32_t V : Vs) {
            if (V % Imax || V > 1984) {
                std::printf("overlap %u does not fit Imax = %u\n", V, Imax);
                return 1;
            }
            const size_t hs = (2048 - V) / Imax, Bs = 2048 / Imax; // slots of a hop and of a segment
            const size_t few = hs > 3 ? hs - 3 : 0;
            const size_t most = (size_t(1) << 40) / (Imax / I.back() > Imax / I.front() ? Imax / I.back() : Imax / I.front());
            const std::vector<std::vector<size_t>> seqs = {
                {0, 1, hs - 1, hs, hs + 1, Bs - 1, Bs, Bs + 1, 3 * Bs + 7},
                {3 * Bs + 7, Bs + 1, Bs, Bs - 1, hs + 1, hs, hs - 1, 1, 0},
                {few, 1, 1, 1, 1, few, 1, 1, 1, 1, 1, 5 * hs + 3},
                {most, 1, hs, size_t(1) << 33},
            };
            for (const auto& seq : seqs)
                for (uint64_t start : {0ull, (1ull << 40) + 3, ~0ull}) check_calls(I, V, start, seq);
            std::vector<size_t> rnd;
            for (int i = 0; i < 200; ++i) rnd.push_back(static_cast<size_t>(rng() % (i % 7 == 0 ? 600 : 12)));
            check_calls(I, V, 12345, rnd);
        }
    }
    std::printf("fft_duc_mixed_plan_check: %llu cases, %llu failures\n", cases, failures);
    return failures ? 1 : 0;
}
