// A stand-alone driver of csrc/hostlogic/duc_position.hpp (the rational Duc's stream position), built with
// -fsanitize=undefined,address by tests/test_duc_rational_ref.py and checked there against Python integers.
// stdin: one case per line, "I D taken next_m next_r n_calls n_1 .. n_calls" (64-bit unsigned decimals).
// stdout: per call "F first taken next_m next_r": the samples the call makes, first() in front of it and the state
// behind it; then, per case, "reset taken next_m next_r" after reset().
#include <cinttypes>
#include <cstdio>

#include "hostlogic/duc_position.hpp"

int main()
{
    gr4pm::hostlogic::DucPosition at;
    unsigned long long I, D, taken, m, r, calls;
    while (std::scanf("%llu %llu %llu %llu %llu %llu", &I, &D, &taken, &m, &r, &calls) == 6) {
        at.I = I, at.D = D, at.taken = taken, at.next_m = m, at.next_r = r;
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
