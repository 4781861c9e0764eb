// A stand-alone driver of csrc/hostlogic/resample_position.hpp (the stream position of the rational Ddc and Duc), built
// with -fsanitize=undefined,address by tests/test_duc_rational_ref.py and checked there against Python integers.
// stdin: one case per line, "I D lead taken next_m next_r n_calls n_1 .. n_calls" (64-bit unsigned decimals).
// stdout: per call "F first taken next_m next_r": the outputs the call makes, first() in front of it and the state
// behind it; then, per case, "reset taken next_m next_r" after reset().
#include <cinttypes>
#include <cstdio>

#include "hostlogic/resample_position.hpp"

int main()
{
    gr4pm::hostlogic::ResamplePosition at;
    unsigned long long I, D, lead, taken, m, r, calls;
    while (std::scanf("%llu %llu %llu %llu %llu %llu %llu", &I, &D, &lead, &taken, &m, &r, &calls) == 7) {
        at.I = I, at.D = D, at.lead = lead, at.taken = taken, at.next_m = m, at.next_r = r;
        for (unsigned long long c = 0; c < calls; ++c) {
            unsigned long long n;
            if (std::scanf("%llu", &n) != 1) return 2;
            const uint64_t first = at.first(), F = at.samples(n);
            at.advance(n, F);
            std::printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", F, first, at.taken, at.next_m, at.next_r);
        }
        at.reset();
        std::printf("reset %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", at.taken, at.next_m, at.next_r);
    }
    return 0;
}
