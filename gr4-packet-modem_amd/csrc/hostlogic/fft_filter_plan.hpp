// hostlogic/fft_filter_plan.hpp -- the integer side of the FftFilter block (fft_filter.hip), HIP-free:
// the validation of a handle's sizes and taps, the arithmetic of a call and of flush(), and the out_cap refusal.
//
// N = 2048, complex taps h[0 .. L - 1] with 1 <= L <= N - 63, an overlap V with L - 1 <= V <= N - 64 (any integer),
// hop = N - V.  x[i] = 0 for i < 0.  Segment s is the N items from s hop - V on and yields out[s hop .. s hop + hop).
//
// The handle sees that as a stream of frames (stream_tail.hpp, keep = V, frame = hop, one row): a virtual stream of V
// zeros and then the samples; segment s is its items [s hop, s hop + N), complete once (s + 1) hop samples were taken.
// Between calls the handle keeps V + (taken mod hop) < N items: the tail, of which `carried` = taken mod hop are samples
// whose outputs are still owed.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace gr4pm {
namespace hostlogic {

constexpr uint32_t kFftFilterN = 2048, kFftFilterMinHop = 64;
constexpr uint32_t kFftFilterMaxOverlap = kFftFilterN - kFftFilterMinHop; // 1984
constexpr uint32_t kFftFilterMaxTaps = kFftFilterMaxOverlap + 1;          // N - 63
constexpr size_t kFftFilterMaxCall = size_t(1) << 40;

// the default overlap: L - 1 rounded up to a multiple of 256, and no more than N - 64 (L - 1 above 1792 rounds to 2048).
// L in 1 .. kFftFilterMaxTaps
constexpr uint32_t fft_filter_default_overlap(size_t L)
{
    const size_t v = (L - 1 + 255) / 256 * 256;
    return static_cast<uint32_t>(v > kFftFilterMaxOverlap ? kFftFilterMaxOverlap : v);
}

enum class FftFilterSizes { ok, no_taps, too_many_taps, overlap_short, overlap_long };

// a handle's L and V (V as the caller gave it; 0 asks for the default)
constexpr FftFilterSizes fft_filter_check_sizes(size_t L, size_t V_asked)
{
    if (L == 0) return FftFilterSizes::no_taps;
    if (L > kFftFilterMaxTaps) return FftFilterSizes::too_many_taps;
    if (V_asked == 0) return FftFilterSizes::ok; // the default overlap of a valid L is valid
    if (V_asked > kFftFilterMaxOverlap) return FftFilterSizes::overlap_long;
    if (V_asked < L - 1) return FftFilterSizes::overlap_short;
    return FftFilterSizes::ok;
}

// set_taps(): the new L against the handle's V, which stays
constexpr FftFilterSizes fft_filter_check_new_taps(size_t L, uint32_t V)
{
    if (L == 0) return FftFilterSizes::no_taps;
    if (L > kFftFilterMaxTaps) return FftFilterSizes::too_many_taps;
    if (L - 1 > V) return FftFilterSizes::overlap_short;
    return FftFilterSizes::ok;
}

// the index of the first tap with a NaN or infinite component, or L when all are finite; taps: L pairs (re, im)
inline size_t fft_filter_first_bad_tap(const float* taps, size_t L)
{
    for (size_t t = 0; t < L; ++t)
        if (!std::isfinite(taps[2 * t]) || !std::isfinite(taps[2 * t + 1])) return t;
    return L;
}

struct FftFilterShape {
    uint32_t overlap; // V
    uint32_t hop;     // N - V
};

constexpr FftFilterShape fft_filter_shape(uint32_t V) { return FftFilterShape{V, kFftFilterN - V}; }

struct FftFilterPlan {
    size_t carried;       // samples taken whose outputs are owed, < hop
    size_t tail;          // H = V + carried: the items in front of the call's
    size_t n_segments;    // the call completes these: its segment i is the items [i hop, i hop + N) of tail ++ input
    size_t samples;       // n_segments hop: what the call delivers
    size_t carried_new;   // (carried + n) mod hop
    size_t tail_new;      // V + carried_new
    uint64_t first_index; // the stream index of the call's first output sample: taken - carried
};

constexpr bool fft_filter_call_fits(size_t n) { return n <= kFftFilterMaxCall; }

// taken: samples before the call; n: the call's (fft_filter_call_fits)
constexpr FftFilterPlan fft_filter_plan(const FftFilterShape& g, uint64_t taken, size_t n)
{
    FftFilterPlan p = {};
    p.carried = static_cast<size_t>(taken % g.hop);
    p.tail = g.overlap + p.carried;
    p.n_segments = (p.carried + n) / g.hop;
    p.samples = p.n_segments * g.hop;
    p.carried_new = (p.carried + n) % g.hop;
    p.tail_new = g.overlap + p.carried_new;
    p.first_index = taken - p.carried;
    return p;
}

// the last item of tail ++ input that segment i of a call reads, plus one
constexpr size_t fft_filter_segment_end(const FftFilterShape& g, size_t i) { return i * g.hop + kFftFilterN; }

// a call that delivers `samples` into room for out_cap is refused
constexpr bool fft_filter_refuses(const FftFilterPlan& p, size_t out_cap) { return p.samples > out_cap; }

struct FftFilterFlush {
    size_t owed;  // samples flush() delivers: carried
    size_t zeros; // the zeros that complete the last segment: hop - carried, or 0 when nothing is owed
};

constexpr FftFilterFlush fft_filter_flush(const FftFilterShape& g, uint64_t taken)
{
    const size_t owed = static_cast<size_t>(taken % g.hop);
    return FftFilterFlush{owed, owed ? g.hop - owed : 0};
}

} // namespace hostlogic
} // namespace gr4pm
