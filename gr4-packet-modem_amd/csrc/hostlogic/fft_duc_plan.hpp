// hostlogic/fft_duc_plan.hpp -- the integer side of the FftDuc block (fft_duc.hip), HIP-free: the
// segment grid and the arithmetic of a call; the validation of a handle's sizes and the default overlap are
// fft_duc_mixed_plan.hpp's, at K equal interpolations.  The nearest bin of a frequency word and
// the response table's word are the FftDdc's (fft_ddc_plan.hpp), used as they are.
//
// N = 2048, I a power of two in 4 .. 64, B = N / I, an overlap V with I | V and L - 1 <= V <= N - 64, hop = N - V,
// hopI = hop / I.  Row k is the items v_k[0], v_k[1], ... over all calls since create or reset, v_k[m] = 0 for m < 0.
// Segment s is the N output samples from
//     a_s = s hop - V
// on (relative to the first output sample), a multiple of I, so it is made of the B items m = a_s / I + n', n' = 0 .. B - 1,
// of every row, and it yields the hop samples s hop .. s hop + hop - 1.
//
// The handle sees that as a stream of frames (stream_tail.hpp): per row a virtual stream of V / I zeros and then the
// items; segment s is the virtual items [s hopI, s hopI + B), complete once (s + 1) hopI items of the row were taken.
// Between calls a row keeps V / I + (taken mod hopI) < B items: the `carried` items.
#pragma once
#include "fft_ddc_plan.hpp"

namespace gr4pm {
namespace hostlogic {

constexpr uint32_t kFftDucN = kFftDdcN;
constexpr uint32_t kFftDucMaxK = 64, kFftDucMinI = 4, kFftDucMaxI = 64, kFftDucMinHop = 64;

// what a handle's I and V fix
struct FftDucShape {
    uint32_t hop;       // N - V: samples of a segment
    uint32_t hop_items; // hopI = hop / I: items per row that complete a segment
    uint32_t keep;      // V / I: items of a segment in front of its hop_items new ones
    uint32_t overlap;   // V
};

constexpr FftDucShape fft_duc_shape(uint32_t I, uint32_t V)
{
    return FftDucShape{kFftDucN - V, (kFftDucN - V) / I, V / I, V};
}

// the absolute index of the first input item of segment s: start_index + a_s, wrapping (the rotator needs it mod 2^32
// only; before the first item it names zeros)
constexpr uint64_t fft_duc_item_index(const FftDucShape& g, uint64_t start_index, uint64_t s)
{
    return start_index + s * g.hop - g.overlap;
}

struct FftDucPlan {
    uint64_t segments_before; // complete before the call
    size_t carried;           // H: items per row in front of the call's, V / I + taken mod hopI < B
    size_t n_segments;        // the call completes these: its segment i is the items [i hopI, i hopI + B) of carried ++ input
    size_t tail_segments;     // the first so many of them begin in the carried items (i hopI < H)
    size_t left;              // items per row the call leaves behind, < B
    size_t samples;           // n_segments hop
};

// taken: items per row before the call; n: the call's
constexpr FftDucPlan fft_duc_plan(const FftDucShape& g, uint64_t taken, size_t n)
{
    FftDucPlan p = {};
    p.segments_before = taken / g.hop_items;
    const size_t pending = static_cast<size_t>(taken - p.segments_before * g.hop_items);
    p.carried = g.keep + pending;
    p.n_segments = (pending + n) / g.hop_items;
    const size_t with_tail = (p.carried + g.hop_items - 1) / g.hop_items;
    p.tail_segments = with_tail < p.n_segments ? with_tail : p.n_segments;
    p.left = p.carried + n - p.n_segments * g.hop_items;
    p.samples = p.n_segments * g.hop;
    return p;
}

} // namespace hostlogic
} // namespace gr4pm
