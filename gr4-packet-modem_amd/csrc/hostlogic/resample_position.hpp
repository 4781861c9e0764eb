// hostlogic/resample_position.hpp -- where a block that resamples by I / D stands in its streams (the rational forms of
// csrc/ddc.hip and csrc/duc.hip, DESIGN.md sections 18 and 19): the input items taken and the next output's newest
// input item and polyphase branch, in 64-bit integers.  Output n of the handle has the upsampled index
// u_n = lead + n D, the newest input item m_n = u_n div I and the branch r_n = u_n mod I; it exists once item m_n has
// arrived.  lead = 0 (the Duc: N items make ceil(N I / D) samples) or D - 1 (the Ddc: floor(N I / D)).  Only (m, r) is
// kept, advanced by (r + F D) divmod I after a call of F outputs: nothing but an item index grows, and the arithmetic
// on it is unsigned and wraps, so the differences below stay right at any stream position.
#pragma once
#include <cstddef>
#include <cstdint>

namespace gr4pm {
namespace hostlogic {

struct ResamplePosition {
    uint64_t I = 1, D = 1; // 1 .. 1024 each, gcd 1
    uint64_t lead = 0;     // the first output's upsampled index: below D
    uint64_t taken = 0;    // input items consumed (per row) since the start
    uint64_t next_m = 0;   // the next output's newest input item, counted from the start: at least `taken` ...
    uint64_t next_r = 0;   // ... and its branch, below I

    void reset()
    {
        taken = 0;
        next_m = lead / I;
        next_r = lead % I;
    }
    // the next output's upsampled index counted from that of the next input item: below I + D
    uint64_t first() const { return (next_m - taken) * I + next_r; }
    // outputs a call of n_in input items completes (n_in I < 2^63): those whose newest item is among them,
    // first() + t D < n_in I
    uint64_t samples(uint64_t n_in) const
    {
        const uint64_t u0 = first(), end = n_in * I;
        return end > u0 ? (end - u0 - 1) / D + 1 : 0;
    }
    // after a call of n_in items that made F = samples(n_in) outputs
    void advance(uint64_t n_in, uint64_t F)
    {
        const uint64_t step = next_r + F * D;
        next_m += step / I;
        next_r = step % I;
        taken += n_in;
    }
};

} // namespace hostlogic
} // namespace gr4pm
