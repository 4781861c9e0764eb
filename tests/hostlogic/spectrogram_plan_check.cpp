// spectrogram_plan_check.cpp -- csrc/hostlogic/spectrogram_plan.hpp (what gr4pm_spectrogram_process runs on the host per
// call) as a stand-alone program for -fsanitize=undefined,address: every hop in 1 .. 2048 x R in {1, 2, 3, 64}, call
// sequences of the lengths {0, 1, hop - 1, hop, N - 1, N, N + 1, 3 N + 7} in several orders.  Asserts that the rows of
// the calls sum to the closed form segments(T) / R, that carry_out of a call is carry_in of the next, that every row
// and every segment of a call is assigned to exactly one wave, which unit reads and which writes the carry, and that no
// segment reads outside tail ++ input.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hostlogic/spectrogram_plan.hpp"

using namespace gr4pm::hostlogic;

static unsigned long long g_calls = 0, g_failures = 0;

#define CHECK(cond)                                                                                                   \
    do {                                                                                                              \
        if (!(cond)) {                                                                                                \
            if (g_failures++ < 20) std::printf("FAIL %s (hop %zu, R %zu, T %llu, n %zu) line %d\n", #cond, hop, R,    \
                                               static_cast<unsigned long long>(T), n, __LINE__);                      \
        }                                                                                                             \
    } while (0)

int main()
{
    const size_t N = 2048;
    const size_t Rs[4] = {1, 2, 3, 64};
    for (size_t hop = 1; hop <= N; ++hop)
        for (size_t R : Rs) {
            const size_t lens[8] = {0, 1, hop - 1, hop, N - 1, N, N + 1, 3 * N + 7};
            for (int order = 0; order < 4; ++order) {
                uint64_t T = 0, total_rows = 0, total_segments = 0;
                size_t carry = 0;
                for (int rep = 0; rep < 2; ++rep)
                    for (int i = 0; i < 8; ++i) {
                        const size_t n = order == 0 ? lens[i] : order == 1 ? lens[7 - i] : order == 2 ? lens[(i * 3) % 8] : lens[(i * 5 + 2) % 8];
                        ++g_calls;
                        for (size_t max_waves : {size_t(1), size_t(8), size_t(2048)}) {
                            const SpectrogramPlan p = spectrogram_plan(T, n, N, hop, R, max_waves);
                            const SpectrumPlan s = spectrum_plan(T, n, N, hop);
                            CHECK(p.seg.segments_before == s.segments_before && p.seg.tail == s.tail && p.seg.n_segments == s.n_segments &&
                                  p.seg.tail_new == s.tail_new);
                            CHECK(p.seg.segments_before == total_segments);
                            // no segment reads outside tail ++ input
                            if (p.seg.n_segments) CHECK((p.seg.n_segments - 1) * hop + N <= p.seg.tail + n);
                            CHECK(p.seg.tail < N && p.seg.tail_new < N);
                            CHECK(p.carry_in == carry && p.carry_in < R && p.carry_out < R);
                            CHECK(p.carry_in + p.seg.n_segments == p.rows * R + p.carry_out);
                            CHECK(p.rows == spectrogram_rows(T + n, N, hop, R) - total_rows);
                            // units: the rows, then the incomplete one
                            CHECK(p.units == (p.seg.n_segments ? p.rows + (p.carry_out ? 1 : 0) : 0));
                            CHECK(p.reads_carry == (p.seg.n_segments != 0 && p.carry_in != 0));
                            CHECK(p.writes_carry == (p.seg.n_segments != 0 && p.carry_out != 0));
                            if (!p.seg.n_segments) CHECK(p.carry_out == p.carry_in && p.waves == 0);
                            CHECK(p.waves <= max_waves && p.run >= 1);
                            if (p.units) CHECK((p.waves - 1) * p.run < p.units && p.units <= p.waves * p.run);
                            // the waves' runs cover every unit once, and the units every segment once, in order
                            size_t next_unit = 0, next_segment = 0;
                            for (size_t w = 0; w < p.waves; ++w) {
                                const size_t u0 = w * p.run, u1 = u0 + p.run < p.units ? u0 + p.run : p.units;
                                CHECK(u0 == next_unit && u1 > u0);
                                for (size_t u = u0; u < u1 && (u < u0 + 3 || u + 3 > u1); ++u) { // both ends of a long run
                                    const size_t a = spectrogram_unit_first(p, R, u), e = spectrogram_unit_end(p, R, u);
                                    CHECK(a < e && e <= p.seg.n_segments);
                                    if (u == u0 && w == 0) CHECK(a == 0);
                                    const size_t before = u == 0 ? p.carry_in : 0; // segments the unit starts from
                                    if (u < p.rows)
                                        CHECK(before + (e - a) == R); // a complete row
                                    else
                                        CHECK(before + (e - a) == p.carry_out && u == p.rows && u + 1 == p.units);
                                    if (u + 1 < p.units) CHECK(spectrogram_unit_first(p, R, u + 1) == e);
                                }
                                if (u0 < u1) {
                                    CHECK(spectrogram_unit_first(p, R, u0) == next_segment);
                                    next_segment = spectrogram_unit_end(p, R, u1 - 1);
                                }
                                next_unit = u1;
                            }
                            CHECK(next_unit == p.units && next_segment == p.seg.n_segments);
                            if (max_waves == 2048) {
                                total_rows += p.rows;
                                total_segments += p.seg.n_segments;
                                carry = p.carry_out;
                            }
                        }
                        T += n;
                        CHECK(total_segments == spectrum_segments(T, N, hop));
                        CHECK(total_rows == total_segments / R && total_rows == (T < N ? 0 : ((T - N) / hop + 1) / R));
                        CHECK(carry == total_segments % R);
                    }
            }
        }
    std::printf("spectrogram_plan_check: %llu calls, %llu failures\n", g_calls, g_failures);
    return g_failures ? 1 : 0;
}
