// Sweeps csrc/hostlogic/row_resample_plan.hpp (the RowResampler's host side) against restatements in
// __int128: a row's output length, the tile the host picks and the span it stages, the index test of the stage, the
// positions of the items that exist, theta, and every refusal of row_plan().  Stand-alone, built with
// -fsanitize=undefined,address by tests/test_row_resample_plan_check.py.
#include "hostlogic/row_resample_plan.hpp"

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

static const i128 kOne = static_cast<i128>(1) << 32;

// the count of m >= 0 with floor((phase0 + m step) / 2^32) <= n + P - 2, uncut
static i128 items_128(i128 n, i128 P, i128 step, i128 phase0)
{
    if (n == 0) return 0;
    const i128 end = (n + P - 1) * kOne; // the first position that is too far
    if (phase0 >= end) return 0;
    return floor_div(end - 1 - phase0, step) + 1;
}

static void check_theta(int32_t freq, uint64_t pos)
{
    const i128 want = floor_div(static_cast<i128>(freq) * static_cast<i128>(pos), kOne);
    const uint32_t w32 = static_cast<uint32_t>(static_cast<uint64_t>(((want % kOne) + kOne) % kOne));
    CHECK(row_theta(freq, pos) == w32, "freq %d pos %llu", freq, static_cast<unsigned long long>(pos));
}

static void check_shape(uint32_t Q, uint64_t P, uint64_t step, uint64_t n, uint64_t phase0, uint64_t n_cols_out)
{
    ++cases;
    const uint64_t lengths[1] = {n};
    const RowRecord rec[1] = {{step, phase0, -12884902}};
    const RowPlan p = row_plan(P, true, n, n, lengths, rec, 1, true, n_cols_out, n_cols_out, true);
    CHECK(p.why == RowRefusal::none, "P %llu step %llu n %llu phase0 %llu: refused with %d", (unsigned long long)P,
          (unsigned long long)step, (unsigned long long)n, (unsigned long long)phase0, static_cast<int>(p.why));
    if (p.why != RowRefusal::none) return;
    // the length
    const i128 full = items_128(n, P, step, phase0);
    if (full > 0) { // by the definition itself: the last item is inside, the next one is not
        const i128 last = floor_div(static_cast<i128>(phase0) + (full - 1) * step, kOne);
        const i128 next = floor_div(static_cast<i128>(phase0) + full * step, kOne);
        CHECK(last <= static_cast<i128>(n) + P - 2 && next > static_cast<i128>(n) + P - 2, "the restatement itself");
    }
    const i128 M128 = full < static_cast<i128>(n_cols_out) ? full : static_cast<i128>(n_cols_out);
    CHECK(static_cast<i128>(p.M[0]) == M128 && p.n[0] == n, "M %u", p.M[0]);
    CHECK(row_output_items(n, P, step, phase0) == static_cast<uint64_t>(full), "row_output_items");
    const uint64_t M = p.M[0];
    // the tile
    const uint32_t T = p.T;
    CHECK(T >= 1 && T <= kRowMaxTile && T == row_tile(P, step), "T %u", T);
    CHECK(row_span_bound(T, step, P) <= kRowStageItems, "T %u: the span bound %llu exceeds the stage", T,
          (unsigned long long)row_span_bound(T, step, P));
    { // the most items whose span fits, by the bound itself; then cut to the workgroup's or a wave's multiple
        i128 most = floor_div(static_cast<i128>(kRowStageItems - P) * kOne, step) + 1;
        CHECK(row_span_bound(static_cast<uint64_t>(most), step, P) <= kRowStageItems &&
                  row_span_bound(static_cast<uint64_t>(most) + 1, step, P) > kRowStageItems, "the restatement of the tile");
        if (most > kRowMaxTile) most = kRowMaxTile;
        if (most >= kRowThreads) most -= most % kRowThreads;
        else if (most >= 64) most -= most % 64;
        CHECK(static_cast<i128>(T) == most, "T %u is not the largest", T);
    }
    CHECK(static_cast<uint64_t>(p.grid_x) * T >= n_cols_out && static_cast<uint64_t>(p.grid_x - 1) * T < n_cols_out && p.grid_y == 1,
          "grid %u", p.grid_x);
    if (M == 0) {
        CHECK(row_tile_items(0, 0, T) == 0, "an empty row has a tile with items");
        return;
    }
    // no position of an item that exists wraps
    const i128 pos_last = static_cast<i128>(phase0) + static_cast<i128>(M - 1) * step;
    CHECK(pos_last < (static_cast<i128>(1) << 64), "the last item's position wraps");
    // tiles: the first ones, the middle, the one of the last item, and one behind it
    const uint64_t tiles = p.grid_x, last_tile = (M - 1) / T;
    const uint64_t pick[] = {0, 1, 2, last_tile / 2, last_tile > 0 ? last_tile - 1 : 0, last_tile, last_tile + 1};
    for (uint64_t t : pick) {
        if (t >= tiles) continue;
        const uint64_t m0 = t * T;
        const uint32_t nv = row_tile_items(m0, M, T);
        const i128 nv128 = static_cast<i128>(m0) >= static_cast<i128>(M) ? 0 : (M - m0 < T ? M - m0 : T);
        CHECK(static_cast<i128>(nv) == nv128, "tile %llu: %u items", (unsigned long long)t, nv);
        if (nv == 0) continue;
        const uint64_t pos0 = phase0 + m0 * step;
        CHECK(static_cast<i128>(pos0) == static_cast<i128>(phase0) + static_cast<i128>(m0) * step, "pos0 wraps");
        const uint64_t span = row_tile_span(pos0, nv, step, P);
        CHECK(span >= P && span <= row_span_bound(T, step, P) && span <= kRowStageItems, "tile %llu: a span of %llu",
              (unsigned long long)t, (unsigned long long)span);
        const i128 base = static_cast<i128>(pos0 >> 32) - static_cast<i128>(P - 1);
        const int64_t base64 = static_cast<int64_t>(pos0 >> 32) - static_cast<int64_t>(P - 1);
        CHECK(static_cast<i128>(base64) == base, "base");
        // every staged index that is admitted lies in [0, n)
        for (uint64_t j = 0; j < span; ++j) {
            const i128 k = base + j;
            const bool in = k >= 0 && k < static_cast<i128>(n);
            CHECK(row_item_loaded(base64 + static_cast<int64_t>(j), n) == in, "stage item %llu", (unsigned long long)j);
        }
        // every index an item needs is a stage item, and admitted exactly when it is in the row
        const uint32_t ms[] = {0, 1, nv / 2, nv - 1};
        for (uint32_t m : ms) {
            if (m >= nv) continue;
            const uint64_t pos = pos0 + static_cast<uint64_t>(m) * step;
            const i128 i = floor_div(static_cast<i128>(phase0) + static_cast<i128>(m0 + m) * step, kOne);
            CHECK(static_cast<i128>(pos >> 32) == i && i <= static_cast<i128>(n) + P - 2, "item %u: i", m);
            for (uint64_t s : {uint64_t(0), uint64_t(1), P / 2, P - 1}) {
                if (s >= P) continue;
                const i128 j = (i - s) - base;
                CHECK(j >= 0 && j < static_cast<i128>(span), "item %u tap %llu reads stage item %lld of %llu", m, (unsigned long long)s,
                      static_cast<long long>(j), (unsigned long long)span);
                const uint32_t idx = static_cast<uint32_t>((pos >> 32) - (pos0 >> 32)) + static_cast<uint32_t>(P - 1) - static_cast<uint32_t>(s);
                CHECK(static_cast<i128>(idx) == j, "the kernel's stage index");
            }
            const uint32_t mu = static_cast<uint32_t>(pos), b = 32 - row_log2(Q);
            CHECK(row_branch(mu, b) < Q && (static_cast<uint64_t>(row_branch(mu, b)) << b) + row_alpha_bits(mu, b) == mu, "branch");
            for (int32_t f : {0, 1, -1, 12884902, -12884902, INT32_MIN, INT32_MAX}) check_theta(f, pos);
        }
    }
}

static void check_refusals()
{
    const uint64_t P = 12, S = uint64_t(1) << 32;
    std::vector<RowRecord> rec(65, RowRecord{S, 0, 0});
    std::vector<uint64_t> len(65, 100);
    auto why = [&](bool x, size_t stride, size_t n_cols, const uint64_t* l, const RowRecord* r, size_t R, bool out, size_t os,
                   uint64_t nco, bool ol) { return row_plan(P, x, stride, n_cols, l, r, R, out, os, nco, ol).why; };
    ++cases;
    CHECK(why(true, 100, 100, len.data(), rec.data(), 64, true, 128, 128, true) == RowRefusal::none, "a good call");
    CHECK(why(true, 100, 100, nullptr, rec.data(), 64, true, 128, 128, true) == RowRefusal::none, "no lengths");
    CHECK(why(true, 100, 100, len.data(), rec.data(), 65, true, 128, 128, true) == RowRefusal::rows, "65 rows");
    CHECK(why(true, 100, 100, len.data(), rec.data(), 0, true, 128, 128, true) == RowRefusal::nothing, "no row");
    CHECK(why(true, 100, 100, len.data(), rec.data(), 2, true, 0, 0, true) == RowRefusal::nothing, "no column");
    CHECK(why(true, 100, 100, len.data(), nullptr, 2, true, 128, 128, true) == RowRefusal::records, "no records");
    CHECK(why(true, 100, 99, len.data(), rec.data(), 2, true, 128, 128, true) == RowRefusal::length, "a long row");
    CHECK(why(true, 99, 100, len.data(), rec.data(), 2, true, 128, 128, true) == RowRefusal::stride, "the input's stride");
    CHECK(why(true, 100, 100, len.data(), rec.data(), 2, true, 127, 128, true) == RowRefusal::stride, "the output's stride");
    CHECK(why(true, 99, 100, len.data(), rec.data(), 1, true, 127, 128, true) == RowRefusal::none, "one row has no stride");
    CHECK(why(true, 100, 100, len.data(), rec.data(), 2, false, 128, 128, true) == RowRefusal::output, "no output");
    CHECK(why(true, 100, 100, len.data(), rec.data(), 2, true, 128, 128, false) == RowRefusal::lengths, "no out_lengths");
    CHECK(why(false, 100, 100, len.data(), rec.data(), 2, true, 128, 128, true) == RowRefusal::input, "no input");
    {
        const uint64_t none[2] = {0, 0};
        CHECK(why(false, 100, 100, none, rec.data(), 2, true, 128, 128, true) == RowRefusal::none, "no input is needed");
    }
    CHECK(why(true, 100, 100, len.data(), rec.data(), 2, true, S, (uint64_t(1) << 31) + 1, true) == RowRefusal::columns, "columns");
    CHECK(why(true, 100, 100, len.data(), rec.data(), 2, true, S, uint64_t(1) << 31, true) == RowRefusal::none, "2^31 columns");
    for (uint64_t bad : {uint64_t(0), kRowMinStep - 1, kRowMaxStep + 1, UINT64_MAX}) {
        rec[1].step = bad;
        CHECK(why(true, 100, 100, len.data(), rec.data(), 2, true, 128, 128, true) == RowRefusal::step, "step %llu",
              (unsigned long long)bad);
    }
    for (uint64_t good : {kRowMinStep, kRowMaxStep}) {
        rec[1].step = good;
        CHECK(why(true, 100, 100, len.data(), rec.data(), 2, true, 128, 128, true) == RowRefusal::none, "step %llu",
              (unsigned long long)good);
    }
    rec[1].step = S;
    rec[1].phase0 = uint64_t(1) << 63;
    CHECK(why(true, 100, 100, len.data(), rec.data(), 2, true, 128, 128, true) == RowRefusal::phase, "phase0 = 2^63");
    rec[1].phase0 = (uint64_t(1) << 63) - 1;
    CHECK(why(true, 100, 100, len.data(), rec.data(), 2, true, 128, 128, true) == RowRefusal::none, "phase0 = 2^63 - 1");
    rec[1].phase0 = 0;
    len[1] = S - P + 1; // n + P - 1 = 2^32
    CHECK(why(true, S, S, len.data(), rec.data(), 2, true, 128, 128, true) == RowRefusal::items, "n + P - 1 = 2^32");
    len[1] = S - P;
    CHECK(why(true, S, S, len.data(), rec.data(), 2, true, 128, 128, true) == RowRefusal::none, "n + P - 1 = 2^32 - 1");
    len[1] = UINT64_MAX;
    CHECK(why(true, UINT64_MAX, UINT64_MAX, len.data(), rec.data(), 2, true, 128, 128, true) == RowRefusal::items, "n = 2^64 - 1");
    // sizes
    for (uint64_t Q : {0, 1, 3, 6, 48, 257, 512}) CHECK(!row_phases_valid(Q), "Q = %llu", (unsigned long long)Q);
    for (uint64_t Q : {2, 4, 32, 256}) CHECK(row_phases_valid(Q) && (uint64_t(1) << row_log2(static_cast<uint32_t>(Q))) == Q, "Q");
    CHECK(row_sizes_valid(256, 16) && !row_sizes_valid(256, 17) && !row_sizes_valid(32, 0) && row_sizes_valid(2, 2048) &&
              !row_sizes_valid(2, 2049), "sizes");
}

int main()
{
    const uint64_t S = uint64_t(1) << 32;
    for (uint32_t Q : {2u, 32u, 256u})
        for (uint64_t P : {uint64_t(1), uint64_t(12), uint64_t(128)}) {
            if (!row_sizes_valid(Q, P)) { // 256 phases of 128 taps: no such handle
                ++cases;
                CHECK(Q * P > kRowMaxTaps, "sizes refused");
                continue;
            }
            for (uint64_t step : {uint64_t(1) << 26, S - 1, S, S + 1, static_cast<uint64_t>(0.893 * 4294967296.0), uint64_t(1) << 38})
                for (uint64_t n : {uint64_t(0), uint64_t(1), P - 1, P, uint64_t(255), uint64_t(5000), S - P})
                    for (uint64_t phase0 : {uint64_t(0), uint64_t(1) << 31, 3 * S + S / 4, (uint64_t(1) << 63) - 1})
                        for (uint64_t cols : {uint64_t(1) << 31, uint64_t(6144), uint64_t(1)}) check_shape(Q, P, step, n, phase0, cols);
        }
    check_refusals();
    std::printf("row_resample_plan_check: %llu cases, %llu failures\n", cases, failures);
    return failures ? 1 : 0;
}
