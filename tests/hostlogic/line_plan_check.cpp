// line_plan_check.cpp -- csrc/hostlogic/line_plan.hpp (the LineSpectrum block's rows, segments and runs) as a stand-alone
// program for -fsanitize=undefined,address.  Every hop in 1 .. 2048 x the lengths 0, 1, hop, N - 1, N, N + 1, 3 N + 7 and
// 64 * 2 * hop + N + 1 x both forms (one segment per transform, pairs):
//   - the runs of a row cover every transform exactly once, in order, with at most 64 each and none empty;
//   - walking the runs as the kernel does, the guarded / unguarded classification never admits an index >= n, every
//     item below n is admitted by a segment, and a segment that does not exist admits nothing;
//   - the eight lengths as the rows of one call: every wave finds its row and run, rows without a segment own no wave.
#include <cstdio>
#include <vector>

#include "hostlogic/line_plan.hpp"

using namespace gr4pm::hostlogic;

static long g_cases = 0, g_failures = 0;

static void fail(const char* what, uint64_t hop, uint64_t n, bool pairs)
{
    if (++g_failures <= 20) std::printf("FAIL %s: hop %llu n %llu pairs %d\n", what, (unsigned long long)hop, (unsigned long long)n, pairs);
}

// the items segment s admits: [i0, end) with end <= n, or nothing
static bool admitted(uint64_t s, uint64_t S, uint64_t hop, uint64_t n, uint64_t* lo, uint64_t* hi)
{
    const uint64_t limit = line_segment_limit(s, S, n), i0 = s * hop;
    bool ok = true;
    if (line_unguarded(i0, limit)) {
        *lo = i0, *hi = i0 + kLineN;
        return *hi <= n;
    }
    // guarded: item i is loaded iff line_item_loaded; the predicate must be monotone and never admit i0 + i >= n
    uint64_t count = 0;
    bool seen_false = false;
    for (uint64_t i = 0; i < kLineN; ++i) {
        const bool ld = line_item_loaded(i0, i, limit);
        if (ld && (i0 + i >= n || seen_false)) ok = false;
        seen_false = seen_false || !ld;
        count += ld;
    }
    *lo = i0, *hi = i0 + count;
    return ok;
}

static void check_row(uint64_t hop, uint64_t n, bool pairs)
{
    ++g_cases;
    const uint64_t S = line_segments(n, hop), T = line_transforms(S, pairs), runs = line_runs(T);
    if ((n == 0) != (S == 0)) fail("segments of an empty row", hop, n, pairs);
    if (S && ((S - 1) * hop + kLineN < n || (S > 1 && (S - 2) * hop + kLineN >= n))) fail("segment count", hop, n, pairs);
    std::vector<unsigned char> visited(T, 0);
    uint64_t covered = 0; // items below this are admitted by some segment
    for (uint64_t run = 0; run < runs; ++run) {
        const uint64_t count = line_run_count(T, run);
        if (count == 0 || count > kLineFloatRun) fail("run length", hop, n, pairs);
        for (uint64_t t = run * kLineFloatRun; t < run * kLineFloatRun + count; ++t) {
            if (t >= T || visited[t]++) {
                fail("transform visited twice or beyond the row", hop, n, pairs);
                continue;
            }
            for (uint64_t s = pairs ? 2 * t : t; s <= (pairs ? 2 * t + 1 : t); ++s) {
                uint64_t lo = 0, hi = 0;
                if (!admitted(s, S, hop, n, &lo, &hi)) fail("an index at or beyond the length is admitted", hop, n, pairs);
                if (s >= S && hi != lo) fail("a segment that does not exist loads", hop, n, pairs);
                if (s < S) {
                    if (lo > covered) fail("items between two segments", hop, n, pairs);
                    if (hi > covered) covered = hi;
                    if (hi != (lo + kLineN < n ? lo + kLineN : n)) fail("a segment's items", hop, n, pairs);
                }
            }
        }
    }
    for (uint64_t t = 0; t < T; ++t)
        if (visited[t] != 1) fail("transform not visited", hop, n, pairs);
    if (covered != n) fail("items not covered", hop, n, pairs);
}

int main()
{
    for (uint64_t hop = 1; hop <= kLineN; ++hop) {
        const uint64_t lengths[8] = {0, 1, hop, kLineN - 1, kLineN, kLineN + 1, 3 * kLineN + 7, 64 * 2 * hop + kLineN + 1};
        for (int pairs = 0; pairs < 2; ++pairs) {
            for (uint64_t n : lengths) check_row(hop, n, pairs != 0);
            // the eight as one call
            ++g_cases;
            const LinePlan p = line_plan(lengths, 8, hop, pairs != 0);
            uint64_t at = 0;
            for (uint32_t r = 0; r < 8; ++r) {
                const uint64_t runs = line_runs(line_transforms(line_segments(lengths[r], hop), pairs != 0));
                if (p.run_start[r] != at) fail("run_start", hop, lengths[r], pairs != 0);
                for (uint64_t w = at; w < at + runs; ++w)
                    if (line_row_of(p.run_start, 8, w) != r) fail("line_row_of", hop, lengths[r], pairs != 0);
                at += runs;
            }
            for (size_t r = 8; r <= kLineMaxRows; ++r)
                if (p.run_start[r] != at) fail("run_start behind the rows", hop, 0, pairs != 0);
        }
    }
    std::printf("line_plan_check: %ld cases, %ld failures\n", g_cases, g_failures);
    return g_failures ? 1 : 0;
}
