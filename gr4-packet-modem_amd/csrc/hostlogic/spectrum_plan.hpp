// hostlogic/spectrum_plan.hpp -- the segment and tail arithmetic of the Spectrum block (spectrum.hip), HIP-free.
//
// The stream is x[0], x[1], ... over all calls since create or reset.  Segment s is x[s hop .. s hop + N), 1 <= hop <= N;
// there is no zero prehistory, so after T samples
//     segments(T) = T < N ? 0 : (T - N) / hop + 1
// exist.  Between calls the handle keeps the samples of the first segment that is not complete yet: with S = segments(T)
// that is x[S hop .. T), fewer than N samples (S hop + N > T by the definition of S), the `tail`.  A call of n samples
// sees the virtual stream tail ++ input, whose item v is x[S hop + v]; the call's segment i (0 <= i < n_segments) is the
// virtual items [i hop, i hop + N), and the new tail is the virtual stream's last tail_new items.
#pragma once
#include <cstddef>
#include <cstdint>

namespace gr4pm {
namespace hostlogic {

inline uint64_t spectrum_segments(uint64_t T, uint64_t N, uint64_t hop) { return T < N ? 0 : (T - N) / hop + 1; }

struct SpectrumPlan {
    uint64_t segments_before; // S: complete before the call
    size_t tail;              // H: items in front of the call's input, T - S hop < N
    size_t n_segments;        // the call completes these
    size_t tail_segments;     // the first so many of them read the tail (segment i does iff i hop < H)
    size_t tail_new;          // items the call leaves behind, < N
};

// T: samples taken before the call; n: the call's
inline SpectrumPlan spectrum_plan(uint64_t T, size_t n, size_t N, size_t hop)
{
    SpectrumPlan p;
    p.segments_before = spectrum_segments(T, N, hop);
    p.tail = static_cast<size_t>(T - p.segments_before * hop);
    p.n_segments = static_cast<size_t>(spectrum_segments(T + n, N, hop) - p.segments_before);
    const size_t with_tail = (p.tail + hop - 1) / hop; // segments i with i hop < H
    p.tail_segments = with_tail < p.n_segments ? with_tail : p.n_segments;
    p.tail_new = p.tail + n - p.n_segments * hop;
    return p;
}

// A call's segments go to waves in runs of `run` consecutive segments (at most float_run: a wave sums its run in
// float32), and the runs to launches of at most max_waves waves, whose partials one buffer holds.
inline size_t spectrum_run(size_t n_segments, size_t waves, size_t float_run)
{
    const size_t even = (n_segments + waves - 1) / waves;
    return even < 1 ? 1 : even > float_run ? float_run : even;
}

} // namespace hostlogic
} // namespace gr4pm
