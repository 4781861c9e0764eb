// spectrum_plan_check.cpp -- csrc/hostlogic/spectrum_plan.hpp (what gr4pm_spectrum_process runs on the host per call) as a
// stand-alone program for -fsanitize=undefined,address: every hop in 1 .. 2048, call sequences of the lengths
// {0, 1, hop - 1, hop, N - 1, N, N + 1, 3 N + 7} in several orders.  Asserts that the segments of the calls sum to the
// closed form T < N ? 0 : (T - N) / hop + 1, that the tail stays below N and is what the definition says, that no segment
// reads outside tail ++ input, that exactly the first tail_segments segments touch the tail, and that the runs of a
// launch cover its segments once with at most float_run segments each.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hostlogic/spectrum_plan.hpp"

using namespace gr4pm::hostlogic;

static unsigned long long g_calls = 0, g_failures = 0;

#define CHECK(cond)                                                                                                   \
    do {                                                                                                              \
        if (!(cond)) {                                                                                                \
            if (g_failures++ < 20) std::printf("FAIL %s (hop %zu, T %llu, n %zu) line %d\n", #cond, hop,              \
                                               static_cast<unsigned long long>(T), n, __LINE__);                      \
        }                                                                                                             \
    } while (0)

int main()
{
    const size_t N = 2048, float_run = 64;
    for (size_t hop = 1; hop <= N; ++hop) {
        const size_t lens[8] = {0, 1, hop - 1, hop, N - 1, N, N + 1, 3 * N + 7};
        for (int order = 0; order < 4; ++order) {
            uint64_t T = 0, total_segments = 0;
            size_t tail = 0;
            for (int rep = 0; rep < 2; ++rep)
                for (int i = 0; i < 8; ++i) {
                    const size_t n = order == 0 ? lens[i] : order == 1 ? lens[7 - i] : order == 2 ? lens[(i * 3) % 8] : lens[(i * 5 + 2) % 8];
                    const SpectrumPlan p = spectrum_plan(T, n, N, hop);
                    ++g_calls;
                    CHECK(p.segments_before == total_segments);
                    CHECK(p.tail == tail && p.tail < N);
                    CHECK(p.tail == T - p.segments_before * hop);
                    // every segment lies inside tail ++ input, and the next one would not
                    if (p.n_segments) CHECK((p.n_segments - 1) * hop + N <= p.tail + n);
                    CHECK(p.n_segments * hop + N > p.tail + n);
                    CHECK(p.tail_segments <= p.n_segments);
                    for (size_t s = 0; s < p.n_segments && s < 4; ++s) CHECK((s * hop < p.tail) == (s < p.tail_segments));
                    if (p.tail_segments < p.n_segments) CHECK(p.tail_segments * hop >= p.tail);
                    if (p.tail_segments) CHECK((p.tail_segments - 1) * hop < p.tail);
                    CHECK(p.tail_new == p.tail + n - p.n_segments * hop && p.tail_new < N);
                    // the launches of the call: runs of at most float_run, every segment once
                    for (size_t max_waves : {size_t(8), size_t(2048)}) {
                        size_t done = 0;
                        while (done < p.n_segments) {
                            const size_t left = p.n_segments - done;
                            const size_t run = spectrum_run(left, max_waves, float_run);
                            CHECK(run >= 1 && run <= float_run);
                            size_t waves = (left + run - 1) / run;
                            if (waves > max_waves) waves = max_waves;
                            const size_t segs = left < waves * run ? left : waves * run;
                            CHECK(segs >= 1 && (waves - 1) * run < segs);
                            done += segs;
                        }
                        CHECK(done == p.n_segments);
                    }
                    T += n;
                    total_segments += p.n_segments;
                    tail = p.tail_new;
                    CHECK(total_segments == spectrum_segments(T, N, hop));
                    CHECK(total_segments == (T < N ? 0 : (T - N) / hop + 1));
                }
        }
    }
    std::printf("spectrum_plan_check: %llu calls, %llu failures\n", g_calls, g_failures);
    return g_failures ? 1 : 0;
}
