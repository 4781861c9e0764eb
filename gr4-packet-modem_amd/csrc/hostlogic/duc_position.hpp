// hostlogic/duc_position.hpp -- where a Duc that resamples by I / D stands in its streams (csrc/duc.hip, DESIGN.md
// section 19): the items taken per row and the next output sample's newest item and polyphase branch, in 64-bit
// integers.  Output sample j of the handle has the upsampled index u_j = j D, the newest item m_j = u_j div I and the
// branch r_j = u_j mod I; it exists once item m_j has arrived, so N items make ceil(N I / D) samples.  Only (m, r) is
// kept, advanced by (r + F D) divmod I after a call of F samples: nothing but an item index grows, and the arithmetic
// on it is unsigned and wraps, so the differences below stay right at any stream position.
#pragma once
#include <cstddef>
#include <cstdint>

namespace gr4pm {
namespace hostlogic {

struct DucPosition {
    uint64_t I = 1, D = 1; // 1 .. 1024 and 1 .. 64, gcd 1
    uint64_t taken = 0;    // items consumed per row since the start
    uint64_t next_m = 0;   // the next sample's newest item, counted from the start: at least `taken` ...
    uint64_t next_r = 0;   // ... and its branch, below I

    void reset() { taken = next_m = next_r = 0; }
    // the next sample's upsampled index counted from that of the next item: below I + D
    uint64_t first() const { return (next_m - taken) * I + next_r; }
    // samples a call of n_in items per row completes (n_in <= 2^31): those whose newest item is among them,
    // first() + t D < n_in I
    uint64_t samples(uint64_t n_in) const
    {
        const uint64_t u0 = first(), end = n_in * I;
        return end > u0 ? (end - u0 - 1) / D + 1 : 0;
    }
    // after a call of n_in items that made F = samples(n_in) samples
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
