// extract_plan_check.cpp -- csrc/hostlogic/extract_plan.hpp on its own (no HIP, no GPU), meant for -fsanitize=undefined,address.
// For D in {1, 2, 5, 16, 1000, 1024} x L in {1, 60, 2000, 8192}, with ddc_geometry()'s tile, several start indices and
// buffers, spans at frame 0, at the buffer's last frame, past its end and at 2^64 / D:
//   * extract_plan() refuses exactly the spans whose indices do not fit, and what it admits keeps every index the
//     kernel forms -- the stage's base and every staged item, restated in 128-bit arithmetic -- within [0, 2^64);
//   * the in-buffer test of every staged index is right: inside the buffer and at or after the handle's start, and then
//     the item it names is the sample's, inside in[0 .. n_in);
//   * every tap of every frame of a tile is a staged item;
//   * burst_span() covers [start_sample, end_sample): every frame whose L samples touch the burst is in the span.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "hostlogic/extract_plan.hpp"
#include "hostlogic/xlate_geometry.hpp"

using namespace gr4pm::hostlogic;
typedef unsigned __int128 u128;
typedef __int128 i128;

static size_t cases = 0, failures = 0;
#define CHECK(cond, ...)                                 \
    do {                                                 \
        if (!(cond)) {                                   \
            if (++failures <= 20) {                      \
                std::printf("FAILED %s: ", #cond);       \
                std::printf(__VA_ARGS__);                \
                std::printf("\n");                       \
            }                                            \
        }                                                \
    } while (0)

static const u128 kTwo64 = u128(1) << 64;

// one admitted call, as k_ddc_extract walks it
static void walk(const ExtractPlan& p, size_t D, size_t L, const DdcTile& tile, uint64_t start, size_t n_in, uint64_t in_index,
                 const std::vector<ExtractSpan>& spans, size_t n_cols)
{
    const unsigned T = tile.T;
    CHECK(p.grid_y == spans.size() && static_cast<uint64_t>(p.grid_x) * T >= n_cols && static_cast<uint64_t>(p.grid_x - 1) * T < n_cols,
          "grid %u x %u for %zu columns of %u", p.grid_x, p.grid_y, n_cols, T);
    CHECK(p.lo <= p.hi && p.skip <= n_in, "lo %llu hi %llu skip %llu", (unsigned long long)p.lo, (unsigned long long)p.hi,
          (unsigned long long)p.skip);
    for (const ExtractSpan& sp : spans) {
        size_t written = 0;
        for (unsigned bx = 0; bx < p.grid_x; ++bx) {
            const uint64_t c0 = static_cast<uint64_t>(bx) * T;
            const unsigned nv = extract_tile_frames(c0, sp.n_frames, T);
            const u128 want = c0 >= sp.n_frames ? 0 : (sp.n_frames - c0 < T ? sp.n_frames - c0 : T);
            CHECK(nv == want, "tile frames %u", nv);
            written += nv;
            if (!nv) continue; // stores zeros, stages nothing
            const u128 f0 = u128(sp.first_frame) + c0;
            for (size_t t0 = 0; t0 < L; t0 += tile.Lc) {
                const size_t lc = L - t0 < tile.Lc ? L - t0 : tile.Lc;
                const i128 vb = i128(L - 1) + i128(f0 * D) + i128(D - 1) - i128(t0 + lc - 1);
                const uint64_t S = extract_stage_items(D, nv, lc);
                CHECK(vb >= 0 && u128(vb) + S <= kTwo64 - 1, "stage base out of 64 bits: D %zu L %zu frame %llu", D, L,
                      (unsigned long long)sp.first_frame);
                const uint64_t base = extract_stage_base(L, D, static_cast<uint64_t>(f0), t0, lc);
                CHECK(u128(base) == u128(vb), "stage base %llu", (unsigned long long)base);
                CHECK(S <= static_cast<uint64_t>(tile.RS) * D, "stage of %llu items, room for %u x %zu", (unsigned long long)S, tile.RS, D);
                // every tap of the first and the last frame of the tile is a staged item, and the sample it should be
                for (unsigned n : {0u, nv - 1})
                    for (size_t t : {t0, t0 + lc - 1}) {
                        const uint64_t item = static_cast<uint64_t>(n) * D + (t0 + lc - 1 - t);
                        CHECK(item < S, "tap %zu of frame %u is item %llu of %llu", t, n, (unsigned long long)item, (unsigned long long)S);
                        CHECK(u128(base) + item == u128(L - 1) + (f0 + n) * D + (D - 1) - t, "tap %zu of frame %u", t, n);
                    }
                // the in-buffer test of the staged items: all of a small stage, else its ends and the buffer's edges
                auto one = [&](uint64_t j) {
                    const uint64_t u = base + j;
                    const i128 a = i128(u) - i128(L - 1) + i128(start); // the absolute index
                    const bool in = a >= i128(start) && a >= i128(in_index) && a < i128(in_index) + i128(n_in);
                    CHECK(extract_in_buffer(u, p.lo, p.hi) == in, "in-buffer test of index %llu: lo %llu hi %llu", (unsigned long long)u,
                          (unsigned long long)p.lo, (unsigned long long)p.hi);
                    if (in && extract_in_buffer(u, p.lo, p.hi)) {
                        const u128 item = u128(u - p.lo) + p.skip;
                        CHECK(item == u128(a - i128(in_index)) && item < n_in, "item of index %llu", (unsigned long long)u);
                    }
                };
                if (S <= 600) {
                    for (uint64_t j = 0; j < S; ++j) one(j);
                } else {
                    for (uint64_t j = 0; j < 64; ++j) one(j), one(S - 1 - j);
                    for (uint64_t edge : {p.lo, p.hi})
                        for (uint64_t d = 0; d < 128; ++d) {
                            const uint64_t u = edge - 64 + d; // may wrap: then it is outside the stage
                            if (u >= base && u - base < S) one(u - base);
                        }
                }
            }
        }
        CHECK(written == sp.n_frames, "%zu frames written of %u", written, sp.n_frames);
    }
}

static void sweep_plans()
{
    const size_t Ds[] = {1, 2, 5, 16, 1000, 1024}, Ls[] = {1, 60, 2000, 8192};
    const size_t n_in = 40000;
    for (size_t D : Ds)
        for (size_t L : Ls) {
            const DdcGeometry geo = ddc_geometry(D, L);
            const unsigned T = geo.tile.T;
            const uint64_t starts[] = {0, 3, (uint64_t(1) << 40) + 3, UINT64_MAX - 3 * n_in};
            for (uint64_t start : starts) {
                std::vector<uint64_t> in_indices = {start, start + 20000, 0, start >= 100 ? start - 100 : 0, start + n_in + 5};
                for (uint64_t in_index : in_indices) {
                    if (in_index > UINT64_MAX - n_in) continue;
                    const uint64_t buf_last = in_index + n_in > start + D ? (in_index + n_in - start) / D - 1 : 0; // last whole frame
                    const uint32_t lens[] = {0, 1, T - 1 ? T - 1 : 1, T, T + 1, 2 * T + 3};
                    const size_t n_cols = 2 * T + 3 + 7;
                    for (uint32_t len : lens) {
                        std::vector<ExtractSpan> spans = {
                            {0, len, 0},                                        // frame 0: the window lies before the start
                            {1, len, buf_last >= len ? buf_last + 1 - len : 0}, // ends at the buffer's last frame
                            {0, len, buf_last},                                 // runs past the buffer's end
                            {1, len, buf_last + 1000},                          // wholly past it
                        };
                        std::vector<ExtractSpan> fit;
                        for (const ExtractSpan& s : spans)
                            if (extract_span_fits(s.first_frame, s.n_frames, D, L, start)) fit.push_back(s);
                        ++cases;
                        if (fit.size() < spans.size()) { // only where start lies at the top of the range
                            const ExtractPlan r = extract_plan(1, 2, D, L, T, start, true, n_in, in_index, spans.data(), spans.size(), true, n_cols, n_cols);
                            CHECK(r.why == ExtractRefusal::overflow && start > (uint64_t(1) << 63), "a span that does not fit was admitted");
                        }
                        if (fit.empty()) continue;
                        const ExtractPlan p = extract_plan(1, 2, D, L, T, start, true, n_in, in_index, fit.data(), fit.size(), true, n_cols, n_cols);
                        CHECK(p.why == ExtractRefusal::none, "refused (%d) what fits", static_cast<int>(p.why));
                        if (p.why == ExtractRefusal::none) walk(p, D, L, geo.tile, start, n_in, in_index, fit, n_cols);
                    }
                    // at 2^64 / D: the last span that fits ends where (first + n) D + max(start, L - 1) = 2^64 - 2 at most
                    const uint64_t most = start > L - 1 ? start : L - 1;
                    const uint64_t end = (UINT64_MAX - 1 - most) / D; // frames [0, end) fit
                    if (end >= T + 2) {
                        std::vector<ExtractSpan> top = {{0, T + 2, end - (T + 2)}};
                        ++cases;
                        const ExtractPlan p = extract_plan(1, 2, D, L, T, start, true, n_in, in_index, top.data(), 1, true, 0, T + 2);
                        CHECK(p.why == ExtractRefusal::none, "the last span that fits was refused");
                        if (p.why == ExtractRefusal::none) walk(p, D, L, geo.tile, start, n_in, in_index, top, T + 2);
                        top[0].first_frame += 1;
                        const ExtractPlan r = extract_plan(1, 2, D, L, T, start, true, n_in, in_index, top.data(), 1, true, 0, T + 2);
                        CHECK(r.why == ExtractRefusal::overflow && r.at == 0, "one frame further was admitted");
                    }
                    for (uint64_t first : {UINT64_MAX / D, UINT64_MAX / D - 1, UINT64_MAX, UINT64_MAX - 1}) {
                        const ExtractSpan s = {0, 2, first};
                        ++cases;
                        const ExtractPlan r = extract_plan(1, 2, D, L, T, start, true, n_in, in_index, &s, 1, true, 0, 2);
                        const bool fits = (u128(first) + 2) * D + most <= kTwo64 - 2;
                        CHECK((r.why == ExtractRefusal::none) == fits && (fits || r.why == ExtractRefusal::overflow), "frame %llu at D %zu",
                              (unsigned long long)first, D);
                        if (r.why == ExtractRefusal::none) walk(r, D, L, geo.tile, start, n_in, in_index, {s}, 2);
                    }
                }
            }
        }
}

static void the_refusals()
{
    const ExtractSpan ok[2] = {{0, 4, 0}, {2, 5, 7}};
    std::vector<ExtractSpan> many(65, ExtractSpan{0, 1, 0});
    auto why = [&](size_t I, size_t K, const ExtractSpan* s, size_t n, bool in, size_t n_in, uint64_t in_index, bool out, size_t stride,
                   size_t n_cols) { return extract_plan(I, K, 5, 60, 256, 0, in, n_in, in_index, s, n, out, stride, n_cols).why; };
    cases += 14;
    CHECK(why(1, 3, ok, 2, true, 100, 0, true, 8, 8) == ExtractRefusal::none, "a good call");
    CHECK(why(2, 3, ok, 2, true, 100, 0, true, 8, 8) == ExtractRefusal::rational, "rational");
    CHECK(why(2, 3, ok, 0, true, 100, 0, true, 8, 8) == ExtractRefusal::rational, "rational, no span");
    CHECK(why(1, 3, ok, 0, true, 100, 0, true, 8, 8) == ExtractRefusal::nothing, "no span");
    CHECK(why(1, 3, ok, 2, true, 100, 0, true, 8, 0) == ExtractRefusal::nothing, "no column");
    CHECK(why(1, 3, many.data(), 65, true, 100, 0, true, 8, 8) == ExtractRefusal::spans, "65 spans");
    CHECK(why(1, 3, many.data(), 64, true, 100, 0, true, 8, 8) == ExtractRefusal::none, "64 spans");
    CHECK(why(1, 3, nullptr, 2, true, 100, 0, true, 8, 8) == ExtractRefusal::spans, "no span array");
    CHECK(why(1, 2, ok, 2, true, 100, 0, true, 8, 8) == ExtractRefusal::channel, "channel 2 of 2");
    CHECK(why(1, 3, ok, 2, true, 100, 0, true, 8, 4) == ExtractRefusal::room, "5 frames in 4 columns");
    CHECK(why(1, 3, ok, 2, true, 100, 0, true, 7, 8) == ExtractRefusal::stride, "stride 7 for 8 columns");
    CHECK(why(1, 3, ok, 1, true, 100, 0, true, 0, 8) == ExtractRefusal::none, "one span: any stride");
    CHECK(why(1, 3, ok, 2, false, 100, 0, true, 8, 8) == ExtractRefusal::input && why(1, 3, ok, 2, false, 0, 0, true, 8, 8) == ExtractRefusal::none,
          "no input array, and none needed");
    CHECK(why(1, 3, ok, 2, true, 100, 0, false, 8, 8) == ExtractRefusal::output && why(1, 3, ok, 2, true, 100, UINT64_MAX - 50, true, 8, 8) == ExtractRefusal::overflow,
          "no output array; a buffer past 2^64");
}

static void sweep_burst_spans()
{
    const uint64_t Ds[] = {1, 2, 5, 16, 1000, 1024}, Ls[] = {1, 60, 2000, 8192};
    const uint64_t starts[] = {0, 3, 12345, (uint64_t(1) << 40) + 3};
    uint64_t rng = 88172645463325252ull;
    auto next = [&]() { return rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17, rng; };
    for (uint64_t D : Ds)
        for (uint64_t L : Ls)
            for (uint64_t start : starts)
                for (int rep = 0; rep < 200; ++rep) {
                    const uint64_t margin = rep % 4 == 0 ? 0 : next() % 1000;
                    // bursts before, across and after the handle's start
                    const uint64_t s = rep % 5 == 0 ? next() % (start + 1) : start + next() % 100000;
                    const uint64_t e = s + (rep % 7 == 0 ? 0 : 1 + next() % 30000);
                    const BurstSpan b = burst_span(s, e, D, L, start, margin);
                    ++cases;
                    if (e <= s) {
                        CHECK(b.n_frames == 0, "an empty burst has frames");
                        continue;
                    }
                    CHECK(b.n_frames >= 1 && extract_span_fits(b.first_frame, b.n_frames, D, L, start), "a span that does not fit");
                    // frame n has the samples [i - L + 1, i], i = start + n D + D - 1: the frames that touch [s, e)
                    const i128 lo_num = i128(s) - i128(start) - i128(D - 1); // n D >= lo_num
                    const i128 n_min = lo_num <= 0 ? 0 : (lo_num + D - 1) / D;
                    const i128 hi_num = i128(e) - 1 - i128(start) - i128(D) + i128(L); // n D <= hi_num
                    if (hi_num < 0) continue; // no frame sees it
                    const i128 n_max = hi_num / D;
                    if (n_max < n_min) continue;
                    CHECK(i128(b.first_frame) <= n_min && i128(b.first_frame) + i128(b.n_frames) - 1 >= n_max,
                          "[%llu, %llu) at D %llu L %llu start %llu: frames %llu + %llu", (unsigned long long)s, (unsigned long long)e,
                          (unsigned long long)D, (unsigned long long)L, (unsigned long long)start, (unsigned long long)b.first_frame,
                          (unsigned long long)b.n_frames);
                    // and the margin is there, where frame 0 does not stop it
                    CHECK(i128(b.first_frame) <= (n_min > i128(margin) ? n_min - i128(margin) : 0) && i128(b.first_frame) + i128(b.n_frames) - 1 >= n_max + i128(margin),
                          "margin %llu", (unsigned long long)margin);
                }
    // at the top of the index range the span is clamped to what fits
    for (uint64_t D : Ds)
        for (uint64_t start : {uint64_t(0), UINT64_MAX - 5, UINT64_MAX - 5000}) {
            const BurstSpan b = burst_span(UINT64_MAX - 4000, UINT64_MAX - 1, D, 60, start, 10);
            ++cases;
            CHECK(b.n_frames == 0 || extract_span_fits(b.first_frame, b.n_frames, D, 60, start), "clamping at D %llu", (unsigned long long)D);
        }
}

int main()
{
    sweep_plans();
    the_refusals();
    sweep_burst_spans();
    std::printf("extract_plan_check: %zu cases, %zu failures\n", cases, failures);
    return failures ? 1 : 0;
}
