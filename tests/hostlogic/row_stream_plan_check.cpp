// Sweeps csrc/hostlogic/row_stream_plan.hpp (the StreamRowResampler's host side) against the
// unbounded definition restated in __int128: the first item behind start_index, the count of a call and of a flush, the
// advance and the rebase over any cutting of a row into calls, the positions and theta of the items, set_row, and every
// refusal of row_stream_plan(); and that a one-shot call is a stream call on a fresh row (check_fresh_row), which is
// what lets k_row_resample and k_row_stream be one body.  Stand-alone, built with -fsanitize=undefined,address by
// tests/test_row_stream_plan_check.py.
//
// theta in 128 bits: floor(freq v / 2^32) mod 2^32 depends on v mod 2^64 only (v + k 2^64 adds freq k 2^32), so the
// restatement reduces pos - ref, which reaches 2^96, to 64 bits before the product with the 32-bit word.
#include "hostlogic/row_stream_plan.hpp"

#include <cstdio>
#include <cstring>
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

static const i128 kOne = static_cast<i128>(1) << 32;
static const i128 kTwo64 = static_cast<i128>(1) << 64;

static i128 floor_div(i128 a, i128 b) // b > 0
{
    i128 q = a / b;
    if (a % b != 0 && a < 0) --q;
    return q;
}
static i128 mod_pos(i128 a, i128 b) { return a - floor_div(a, b) * b; }

// the unbounded definition of one row
struct Def {
    i128 step, next_pos, next_m; // the next output item
    i128 A;                      // items taken
    i128 ref;
    uint32_t phi;
    int32_t freq;
    i128 phase0, start;

    void create()
    {
        A = start, ref = 0, phi = 0;
        next_m = phase0 >= start * kOne ? 0 : floor_div(start * kOne - phase0 + step - 1, step);
        next_pos = phase0 + next_m * step;
    }
    uint32_t theta(i128 pos) const
    {
        const i128 v = mod_pos(pos - ref, kTwo64);
        return phi + static_cast<uint32_t>(static_cast<uint64_t>(mod_pos(floor_div(static_cast<i128>(freq) * v, kOne), kOne)));
    }
    i128 count(i128 last_item) const // the items not yet made with floor(pos) <= last_item
    {
        const i128 end = (last_item + 1) * kOne; // the first position that is too far
        return next_pos >= end ? 0 : floor_div(end - 1 - next_pos, step) + 1;
    }
    void set_row(i128 new_step, int32_t new_freq)
    {
        phi = theta(next_pos), ref = next_pos, freq = new_freq, step = new_step;
    }
};

static RowStreamRow make_row(uint64_t step, uint64_t phase0, uint64_t start, int32_t freq)
{
    RowStreamRow s = {};
    s.step = step, s.phase0 = phase0, s.start = start, s.freq = freq;
    row_stream_start(s);
    return s;
}

static void check_created(const RowStreamRow& s, const Def& d)
{
    CHECK(s.items_in == static_cast<uint64_t>(d.A), "A at create");
    CHECK(s.items_out == static_cast<uint64_t>(mod_pos(d.next_m, kTwo64)), "the first item's index: %llu",
          static_cast<unsigned long long>(s.items_out));
    CHECK(static_cast<i128>(s.d) == d.next_pos - d.A * kOne, "the first item's position");
    CHECK(d.next_pos >= d.start * kOne && (d.next_m == 0 || d.next_pos - d.step < d.start * kOne), "the restatement itself");
    CHECK(s.d < (uint64_t(1) << 63), "d at create");
}

// the items of a call (or of a flush: n = 0, span = P - 1) against the definition, before either side advances
static void check_items(const RowStreamRow& s, const Def& d, uint64_t n, uint64_t span, uint64_t P, uint32_t Q, uint64_t M)
{
    const i128 want = d.count(d.A + static_cast<i128>(span) - 1);
    CHECK(static_cast<i128>(M) == want, "a count of %llu", static_cast<unsigned long long>(M));
    CHECK(row_stream_items_valid(n, P), "the call's length");
    if (M == 0) return;
    const uint32_t b = 32 - row_log2(Q);
    for (uint64_t k : {uint64_t(0), uint64_t(1), M / 2, M - 1}) {
        if (k >= M) continue;
        const uint64_t rel = s.d + k * s.step;
        const i128 rel128 = static_cast<i128>(s.d) + static_cast<i128>(k) * static_cast<i128>(s.step);
        const i128 pos = d.next_pos + static_cast<i128>(k) * d.step;
        CHECK(static_cast<i128>(rel) == rel128 && d.A * kOne + rel128 == pos, "item %llu: its position", static_cast<unsigned long long>(k));
        // the stage's origin is item A - (P - 1): that position does not wrap either, and the newest item is in the span
        CHECK(rel128 + static_cast<i128>(P - 1) * kOne < kTwo64, "the stage position wraps");
        CHECK(floor_div(rel128, kOne) <= static_cast<i128>(span) - 1, "item %llu is too far", static_cast<unsigned long long>(k));
        // the rotator's operand: positive (the position never precedes ref), unwrapped, and theta is the definition's
        const i128 tp = rel128 + kOne - static_cast<i128>(s.ref_frac);
        CHECK(tp > 0 && tp < kTwo64 && static_cast<i128>(row_stream_theta_pos(rel, s.ref_frac)) == tp, "the rotator's operand");
        CHECK(row_stream_theta(s, rel) == d.theta(pos), "item %llu: theta %u, defined %u", static_cast<unsigned long long>(k),
              row_stream_theta(s, rel), d.theta(pos));
        const uint32_t mu = static_cast<uint32_t>(rel);
        CHECK(static_cast<i128>(mu) == mod_pos(pos, kOne) && row_branch(mu, b) < Q, "the fraction");
        // the sources of the taps: history below 0, the call's items in [0, n), +0 behind
        const i128 i = floor_div(rel128, kOne);
        for (uint64_t t : {uint64_t(0), P / 2, P - 1}) {
            const i128 idx = i - static_cast<i128>(t);
            const RowStreamSource src = row_stream_source(static_cast<int64_t>(idx), n);
            CHECK(idx >= -static_cast<i128>(P - 1), "a tap in front of the history");
            CHECK(src == (idx < 0 ? RowStreamSource::history : idx < static_cast<i128>(n) ? RowStreamSource::input : RowStreamSource::zero),
                  "a tap's source");
        }
    }
    // the item behind the last one is too far
    const i128 next = static_cast<i128>(s.d) + static_cast<i128>(M) * static_cast<i128>(s.step);
    CHECK(floor_div(next, kOne) > static_cast<i128>(span) - 1, "the count is not the largest");
}

static void advance_both(RowStreamRow& s, Def& d, uint64_t n, uint64_t M)
{
    const uint32_t hist = s.hist;
    row_stream_advance(s, n, M);
    d.next_pos += static_cast<i128>(M) * d.step, d.next_m += M, d.A += n;
    CHECK(s.items_in == static_cast<uint64_t>(mod_pos(d.A, kTwo64)) && s.items_out == static_cast<uint64_t>(mod_pos(d.next_m, kTwo64)),
          "the counters");
    CHECK(static_cast<i128>(s.d) == d.next_pos - d.A * kOne && s.d < (uint64_t(1) << 63), "d behind a call");
    CHECK(s.hist == (n ? hist ^ 1u : hist), "the history buffer");
}

static uint64_t feed(RowStreamRow& s, Def& d, const std::vector<uint64_t>& cut, uint64_t P, uint32_t Q, size_t retune_at,
                     uint64_t new_step, int32_t new_freq)
{
    uint64_t total = 0;
    for (size_t c = 0; c < cut.size(); ++c) {
        if (c == retune_at) {
            const uint64_t d0 = s.d;
            const uint32_t before = row_stream_theta(s, s.d);
            CHECK(before == d.theta(d.next_pos), "theta in front of set_row");
            row_stream_retune(s, new_step, new_freq);
            d.set_row(new_step, new_freq);
            CHECK(s.d == d0, "set_row moves p*");
            CHECK(row_stream_theta(s, s.d) == before && d.theta(d.next_pos) == before, "set_row: the phase at p* is not kept");
        }
        const uint64_t n = cut[c];
        const uint64_t M = row_stream_count(s, n);
        check_items(s, d, n, n, P, Q, M);
        advance_both(s, d, n, M);
        total += M;
    }
    const uint64_t F = row_stream_flush_count(s, P);
    check_items(s, d, 0, P - 1, P, Q, F);
    return total + F;
}

static std::vector<std::vector<uint64_t>> cuttings(uint64_t P)
{
    const uint64_t N = 2 * P + 700, pm2 = P >= 2 ? P - 2 : 0;
    std::vector<std::vector<uint64_t>> cuts;
    auto rest = [&](std::vector<uint64_t> v) {
        uint64_t sum = 0;
        for (uint64_t n : v) sum += n;
        v.push_back(N - sum);
        cuts.push_back(v);
    };
    cuts.push_back({N});
    rest({0});
    rest({1});
    rest({pm2});
    rest({P - 1});
    rest({P});
    rest({N - 1});
    {
        std::vector<uint64_t> v(40, 1);
        for (uint64_t n : {pm2, P - 1, P, uint64_t(0), uint64_t(255), uint64_t(257)}) v.push_back(n);
        rest(v);
    }
    cuts.push_back(std::vector<uint64_t>(N, 1));
    {
        std::vector<uint64_t> v;
        for (int i = 0; i < 50; ++i) v.push_back(0), v.push_back(7);
        rest(v);
    }
    {
        std::vector<uint64_t> v;
        uint64_t sum = 0, lcg = 12345;
        while (sum < N) {
            lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
            uint64_t n = (lcg >> 33) % (2 * P + 3);
            if (n > N - sum) n = N - sum;
            v.push_back(n), sum += n;
        }
        cuts.push_back(v);
    }
    rest({P - 1, P - 1, pm2, 1, 0, 0, P});
    return cuts;
}

static void check_case(uint32_t Q, uint64_t P, uint64_t step, uint64_t start, uint64_t phase0, const std::vector<uint64_t>& cut,
                       bool retune)
{
    ++cases;
    const int32_t freq = -12884902;
    RowStreamRow s = make_row(step, phase0, start, freq);
    Def d = {};
    d.step = step, d.phase0 = phase0, d.start = start, d.freq = freq;
    d.create();
    check_created(s, d);
    const uint64_t new_step = step == kRowMaxStep ? kRowMinStep + 12345 : step + (step >> 3) + 1 > kRowMaxStep ? kRowMaxStep : step + (step >> 3) + 1;
    const uint64_t total = feed(s, d, cut, P, Q, retune ? cut.size() / 2 : cut.size() + 1, new_step, 3 << 20);
    if (retune) return;
    // the cutting's counts sum to the count of one call, and the state behind it is that call's
    uint64_t N = 0;
    for (uint64_t n : cut) N += n;
    RowStreamRow one = make_row(step, phase0, start, freq);
    const uint64_t M1 = row_stream_count(one, N);
    row_stream_advance(one, N, M1);
    CHECK(M1 + row_stream_flush_count(one, P) == total, "the cutting makes %llu items, one call %llu", static_cast<unsigned long long>(total),
          static_cast<unsigned long long>(M1 + row_stream_flush_count(one, P)));
    CHECK(one.d == s.d && one.phi == s.phi && one.ref_frac == s.ref_frac && one.items_in == s.items_in && one.items_out == s.items_out,
          "the state behind the cutting");
    // and with nothing in front of the row, to the one-shot block's M_r
    if (start == 0) CHECK(total == row_output_items(N, P, step, phase0), "the one-shot's count");
    // back to the created state
    row_stream_start(s);
    const RowStreamRow again = make_row(step, phase0, start, freq);
    CHECK(s.d == again.d && s.phi == again.phi && s.items_in == again.items_in && s.items_out == again.items_out && s.ref_frac == 0,
          "the state behind a restart");
}

// calls of the largest length, one after the other: nothing wraps
static void check_long(uint32_t Q, uint64_t P, uint64_t step, uint64_t start)
{
    ++cases;
    RowStreamRow s = make_row(step, 5, start, 12345678);
    Def d = {};
    d.step = step, d.phase0 = 5, d.start = start, d.freq = 12345678;
    d.create();
    const uint64_t n = (uint64_t(1) << 32) - P;
    CHECK(!row_stream_items_valid(n + 1, P) && !row_stream_items_valid(UINT64_MAX, P), "a length that is too long");
    for (int call = 0; call < 3; ++call) {
        const uint64_t M = row_stream_count(s, n);
        check_items(s, d, n, n, P, Q, M);
        advance_both(s, d, n, M);
    }
}

static void check_div()
{
    ++cases;
    for (uint64_t step : {kRowMinStep, kRowMinStep + 1, (uint64_t(1) << 32) - 1, uint64_t(1) << 32, kRowMaxStep - 1, kRowMaxStep})
        for (uint64_t hi : {uint64_t(0), uint64_t(1), uint64_t(0xffffffffu), (uint64_t(1) << 63) - 1, uint64_t(1) << 63, UINT64_MAX})
            for (uint32_t lo : {0u, 1u, 0x80000000u, 0xffffffffu}) {
                const unsigned __int128 v = (static_cast<unsigned __int128>(hi) << 32) | lo;
                const RowDiv q = row_div96(hi, lo, step);
                CHECK(q.quot == static_cast<uint64_t>(v / step) && q.rem == static_cast<uint64_t>(v % step), "row_div96");
            }
}

static void check_refusals()
{
    ++cases;
    const uint64_t P = 12, S = uint64_t(1) << 32;
    std::vector<RowStreamRow> rows(64, make_row(S, 0, 0, 7));
    rows[1] = make_row(S / 2, 0, 0, 7); // two items per input item
    const std::vector<RowStreamRow> before = rows;
    std::vector<uint64_t> len(64, 100);
    auto why = [&](bool flush, bool x, size_t stride, size_t n_cols, const uint64_t* l, size_t R, bool out, size_t os, uint64_t nco,
                   bool ol) {
        const RowStreamPlan p = row_stream_plan(rows.data(), R, P, flush, x, stride, n_cols, l, out, os, nco, ol);
        CHECK(std::memcmp(rows.data(), before.data(), rows.size() * sizeof rows[0]) == 0, "a plan changes the state");
        return p;
    };
    RowStreamPlan p = why(false, true, 100, 100, len.data(), 64, true, 200, 200, true);
    CHECK(p.why == RowStreamRefusal::none && p.M[0] == 100 && p.M[1] == 200 && p.n[5] == 100 && p.grid_y == 64 &&
              p.T == row_tile(P, S) && static_cast<uint64_t>(p.grid_x) * p.T >= 200, "a good call");
    CHECK(why(false, true, 100, 100, nullptr, 64, true, 200, 200, true).why == RowStreamRefusal::none, "no lengths");
    p = why(false, true, 100, 100, len.data(), 64, true, 200, 199, true);
    CHECK(p.why == RowStreamRefusal::room && p.at == 1, "one column too few");
    CHECK(why(false, true, 100, 99, len.data(), 2, true, 200, 200, true).why == RowStreamRefusal::length, "a long row");
    CHECK(why(false, true, 99, 100, len.data(), 2, true, 200, 200, true).why == RowStreamRefusal::stride, "the input's stride");
    CHECK(why(false, true, 100, 100, len.data(), 2, true, 199, 200, true).why == RowStreamRefusal::stride, "the output's stride");
    CHECK(why(false, true, 99, 100, len.data(), 1, true, 99, 100, true).why == RowStreamRefusal::none, "one row has no stride");
    CHECK(why(false, true, 100, 100, len.data(), 2, false, 200, 200, true).why == RowStreamRefusal::output, "no output");
    CHECK(why(false, true, 100, 100, len.data(), 2, true, 200, 200, false).why == RowStreamRefusal::lengths, "no out_lengths");
    CHECK(why(false, false, 100, 100, len.data(), 2, true, 200, 200, true).why == RowStreamRefusal::input, "no input");
    CHECK(why(false, true, 100, 100, len.data(), 2, true, S, (uint64_t(1) << 31) + 1, true).why == RowStreamRefusal::columns, "columns");
    {
        const uint64_t none[2] = {0, 0};
        p = why(false, false, 100, 100, none, 2, false, 0, 0, true);
        CHECK(p.why == RowStreamRefusal::none && p.grid_x == 0, "nothing in, nothing out");
        const uint64_t big[2] = {100, S - P + 1};
        CHECK(why(false, true, S, S, big, 2, true, S, uint64_t(1) << 31, true).why == RowStreamRefusal::items, "n + P - 1 = 2^32");
        const uint64_t most[2] = {100, S - P};
        CHECK(why(false, true, S, S, most, 2, true, S, uint64_t(1) << 31, true).why == RowStreamRefusal::room, "2^33 items in a call");
    }
    // a flush: P - 1 = 11 further items, so 11 and 22 items
    p = why(true, false, 0, 0, nullptr, 2, true, 22, 22, true);
    CHECK(p.why == RowStreamRefusal::none && p.M[0] == 11 && p.M[1] == 22 && p.n[0] == 0 && p.n[1] == 0, "a flush");
    CHECK(why(true, false, 0, 0, nullptr, 2, true, 22, 21, true).why == RowStreamRefusal::room, "a flush with a column too few");
    CHECK(why(true, false, 0, 0, nullptr, 2, false, 22, 22, true).why == RowStreamRefusal::output, "a flush without output");
}

// the one-shot call is a stream call on a fresh row (start = 0): the state the one-shot host code hands the shared kernel
// body, the rotator's operand in either form, and the count of a row of n > 0 items; a row of no items makes nothing
// whatever the stream's count over P - 1 items is, which is why the one-shot host code keeps row_output_items()
static void check_fresh_row()
{
    const uint64_t S = uint64_t(1) << 32;
    uint64_t lcg = 2024;
    auto rnd = [&] {
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        return lcg >> 11;
    };
    std::vector<int32_t> words = {0, 1, -1, INT32_MAX, INT32_MIN, INT32_MIN + 1, 12884902, -12884902};
    for (int i = 0; i < 8; ++i) words.push_back(static_cast<int32_t>(static_cast<uint32_t>(rnd())));
    for (uint64_t P : {uint64_t(1), uint64_t(2), uint64_t(12), uint64_t(2048)})
        for (uint64_t step : {kRowMinStep, kRowMinStep + 1, S - 1, S, S + 1, static_cast<uint64_t>(2.27 * 4294967296.0), kRowMaxStep - 1, kRowMaxStep})
            for (uint64_t phase0 : {uint64_t(0), uint64_t(1), S / 2 + 3, S - 1, (P + 5) * S + S / 4, (uint64_t(1) << 63) - 1})
                for (uint64_t n : {uint64_t(0), uint64_t(1), P - 1, P, S - P})
                    for (int32_t freq : words) {
                        ++cases;
                        const RowStreamRow s = make_row(step, phase0, 0, freq);
                        CHECK(s.d == phase0 && s.ref_frac == 0 && s.items_out == 0 && s.items_in == 0 && s.hist == 0, "the fresh row");
                        CHECK(s.phi == 0u - static_cast<uint32_t>(freq), "the fresh row's Phi");
                        CHECK(row_stream_items_valid(n, P), "the row's length");
                        const uint64_t span = n + P - 1, M = row_output_items(n, P, step, phase0);
                        if (n == 0) {
                            CHECK(M == 0, "a row of no items makes %llu", static_cast<unsigned long long>(M));
                            continue;
                        }
                        CHECK(M == row_stream_count(s, span), "the one-shot's count %llu, the stream's %llu",
                              static_cast<unsigned long long>(M), static_cast<unsigned long long>(row_stream_count(s, span)));
                        // positions below (n + P - 1) 2^32: the first, the last and random ones, whether an item sits there or not
                        const uint64_t end = span << 32;
                        uint64_t at[8] = {0, end - 1, phase0 < end ? phase0 : 0, M ? phase0 + (M - 1) * step : 0};
                        for (int i = 4; i < 8; ++i) at[i] = (rnd() << 11 | (rnd() & 0x7ffu)) % end;
                        for (uint64_t pos : at) {
                            CHECK(pos < end && static_cast<i128>(row_stream_theta_pos(pos, s.ref_frac)) == static_cast<i128>(pos) + kOne,
                                  "the carried operand wraps");
                            CHECK(row_stream_theta(s, pos) == row_theta(freq, pos), "theta at %llu: carried %u, one-shot %u",
                                  static_cast<unsigned long long>(pos), row_stream_theta(s, pos), row_theta(freq, pos));
                        }
                    }
}

int main()
{
    const uint64_t S = uint64_t(1) << 32;
    check_div();
    check_refusals();
    check_fresh_row();
    for (uint32_t Q : {2u, 32u, 256u})
        for (uint64_t P : {uint64_t(1), uint64_t(12), uint64_t(128)}) {
            if (!row_sizes_valid(Q, P)) { // 256 phases of 128 taps: no such handle
                ++cases;
                CHECK(Q * P > kRowMaxTaps, "sizes refused");
                continue;
            }
            const std::vector<std::vector<uint64_t>> cuts = cuttings(P);
            CHECK(cuts.size() >= 12, "a dozen cuttings");
            for (uint64_t step : {uint64_t(1) << 26, S - 1, S, S + 1, static_cast<uint64_t>(2.27 * 4294967296.0), uint64_t(1) << 38})
                for (uint64_t start : {uint64_t(0), uint64_t(1), S - 1, 2 * S + 20480, uint64_t(1) << 63}) {
                    for (uint64_t phase0 : {uint64_t(0), 3 * S + S / 4, (uint64_t(1) << 63) - 1})
                        for (size_t c = 0; c < cuts.size(); ++c) {
                            check_case(Q, P, step, start, phase0, cuts[c], false);
                            if (cuts[c].size() >= 2) check_case(Q, P, step, start, phase0, cuts[c], true);
                        }
                    check_long(Q, P, step, start);
                }
        }
    std::printf("row_stream_plan_check: %llu cases, %llu failures\n", cases, failures);
    return failures ? 1 : 0;
}
