// hostlogic/fft_ddc_plan.hpp -- the integer side of the FftDdc block (fft_ddc.hip), HIP-free: the
// nearest bin of a frequency word, the rotator's phase and the segment and tail arithmetic of a call.  The validation of a
// handle's sizes and the default overlap are fft_ddc_mixed_plan.hpp's, at K equal decimations.
//
// N = 2048, D a power of two in 4 .. 64, B = N / D, an overlap V with D | V and L - 1 <= V <= N - 64, hop = N - V.  The
// stream is x[0], x[1], ... over all calls since create or reset, x[i] = 0 for i < 0.  Segment s is the N items from
//     a_s = s hop - V + D - 1
// on, and it yields the hop / D frames n = s hop / D + (n' - V / D), n' = V / D .. B - 1, whose newest sample is
// a_s + n' D = n D + D - 1: the Ddc's own frame grid.
//
// The handle sees that as the Spectrum's arithmetic (spectrum_plan.hpp) on a virtual stream: Z = V - D + 1 zeros in front
// of x when V >= D, or x without its first D - 1 samples when V = 0 (then L = 1 and frame n is h[0] x[n D + D - 1]: the
// samples in front of D - 1 belong to no frame).  Segment s is the virtual items [s hop, s hop + N).  Between calls the
// handle keeps the virtual items of the first segment that is not complete yet, fewer than N: the `tail`, V carried
// samples plus the incomplete hop.
#pragma once
#include <cstddef>
#include <cstdint>

namespace gr4pm {
namespace hostlogic {

constexpr uint32_t kFftDdcN = 2048;
constexpr uint32_t kFftDdcMaxK = 64, kFftDdcMinD = 4, kFftDdcMaxD = 64, kFftDdcMinHop = 64;

// c = floor(w N / 2^32 + 1 / 2) mod N: w / 2^21 rounded half up, in integers
constexpr uint32_t fft_ddc_bin(uint32_t w)
{
    return static_cast<uint32_t>(((static_cast<uint64_t>(w) + (1u << 20)) >> 21) & (kFftDdcN - 1));
}

// phi = (w i - c 2^21 p) mod 2^32: the phase of the Ddc's mixer at the absolute index i, less what the slice's shift
// by c bins has turned at item p of the segment already.  Wrapping 32-bit arithmetic is exact: every term is an integer
// and only phi mod 2^32 matters.
constexpr uint32_t fft_ddc_phi(uint32_t w, uint32_t c, uint64_t i, uint32_t p)
{
    return w * static_cast<uint32_t>(i) - (c << 21) * p;
}

// psi = ((c + u) 2^21 - w) mod 2^32: the response table's frequency (c + u) / N - w / 2^32 as a word
constexpr uint32_t fft_ddc_table_word(uint32_t w, uint32_t c, int32_t u)
{
    return ((c + static_cast<uint32_t>(u)) << 21) - w;
}

constexpr bool fft_ddc_pow2(uint64_t v) { return v != 0 && (v & (v - 1)) == 0; }

// what a handle's D and V fix
struct FftDdcShape {
    uint32_t hop;    // N - V
    uint32_t frames; // hop / D: frames of a segment
    uint32_t first;  // V / D: the first n' that is kept
    uint32_t zeros;  // Z: zeros in front of the stream
    uint32_t skip;   // samples of the stream in front of the virtual stream (V = 0 only)
};

constexpr FftDdcShape fft_ddc_shape(uint32_t D, uint32_t V)
{
    return FftDdcShape{kFftDdcN - V, (kFftDdcN - V) / D, V / D, V >= D ? V - D + 1 : 0, V >= D ? 0 : D - 1 - V};
}

// virtual items after `taken` samples of the stream
constexpr uint64_t fft_ddc_virtual(const FftDdcShape& g, uint64_t taken)
{
    return g.zeros + (taken > g.skip ? taken - g.skip : 0);
}

// segments complete after T virtual items
constexpr uint64_t fft_ddc_complete(const FftDdcShape& g, uint64_t T)
{
    return T < kFftDdcN ? 0 : (T - kFftDdcN) / g.hop + 1;
}

// the absolute index of item 0 of segment s: start_index + a_s, wrapping (the rotator needs it mod 2^32 only)
constexpr uint64_t fft_ddc_segment_index(const FftDdcShape& g, uint64_t start_index, uint64_t s)
{
    return start_index + s * g.hop - g.zeros + g.skip;
}

struct FftDdcPlan {
    size_t drop;              // samples at the front of the call's input that belong to no frame (V = 0 only)
    size_t n_used;            // n - drop: what the call adds to the virtual stream
    uint64_t segments_before; // S: complete before the call
    size_t tail;              // H: virtual items in front of the call's, < N
    size_t n_segments;        // the call completes these: its segment i is the items [i hop, i hop + N) of tail ++ input
    size_t tail_segments;     // the first so many of them begin in the carried items (i hop < H)
    size_t tail_new;          // virtual items the call leaves behind, < N
    size_t frames;            // n_segments hop / D
};

// taken: samples of the stream before the call; n: the call's
constexpr FftDdcPlan fft_ddc_plan(const FftDdcShape& g, uint64_t taken, size_t n)
{
    FftDdcPlan p = {};
    const uint64_t skip_left = taken < g.skip ? g.skip - taken : 0;
    p.drop = static_cast<size_t>(skip_left < n ? skip_left : n);
    p.n_used = n - p.drop;
    const uint64_t T = fft_ddc_virtual(g, taken);
    p.segments_before = fft_ddc_complete(g, T);
    p.tail = static_cast<size_t>(T - p.segments_before * g.hop);
    p.n_segments = static_cast<size_t>(fft_ddc_complete(g, T + p.n_used) - p.segments_before);
    const size_t with_tail = (p.tail + g.hop - 1) / g.hop;
    p.tail_segments = with_tail < p.n_segments ? with_tail : p.n_segments;
    p.tail_new = p.tail + p.n_used - p.n_segments * g.hop;
    p.frames = p.n_segments * g.frames;
    return p;
}

} // namespace hostlogic
} // namespace gr4pm
