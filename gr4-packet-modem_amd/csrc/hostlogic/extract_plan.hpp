// hostlogic/extract_plan.hpp -- the host side of gr4pm_ddc_extract (csrc/ddc.hip), HIP-free: one
// function that validates a call and sizes its launch, the index expressions k_ddc_extract stages by, and burst_span(),
// which turns a burst's samples into the frames that see them.  tests/hostlogic/extract_plan_check.cpp sweeps them.
//
// Indices.  Frame n of a handle has the newest sample i = start_index + n D + D - 1 and takes tap t from sample i - t.
// The kernel counts samples from L - 1 before the handle's start, u = (absolute index) - start_index + (L - 1), so that
// the oldest sample of frame 0, u = D - 1, is not negative: every index it forms is an unsigned 64-bit number, and
// extract_plan() refuses a span whose last frame would carry one past 2^64 - 2.  The buffer of a call is the range
// [lo, hi) of u: a sample inside it is in[u - lo] of the pointer the kernel gets (the host skips what lies before the
// handle's start, where the stream is zero by definition), every other sample is zero.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../../include/gr4pm_hip.h"

namespace gr4pm {
namespace hostlogic {

using ExtractSpan = gr4pm_ddc_span; // channel, n_frames, first_frame

constexpr size_t kMaxExtractSpans = 64; // of a call: they travel by value, 16 bytes each

enum class ExtractRefusal {
    none,      // launch `grid`
    nothing,   // no span or no column: OK, nothing to do
    rational,  // interpolation > 1
    spans,     // more than kMaxExtractSpans, or no span array
    channel,   // spans[at].channel >= K
    room,      // spans[at].n_frames > n_cols
    stride,    // n_spans > 1 and out_stride < n_cols
    overflow,  // spans[at] reaches a sample index beyond 64 bits; or the buffer's end does; or the grid is too wide
    input,     // no input array for n_in > 0
    output,    // no output array
};

struct ExtractPlan {
    ExtractRefusal why;
    size_t at;              // the span a refusal names
    unsigned grid_x, grid_y; // tiles of T columns, spans
    uint64_t lo, hi;        // the buffer in the kernel's indices: empty when lo == hi
    uint64_t skip;          // items of `in` that lie before lo: the kernel's pointer is in + skip
};

// the kernel's index of the stage's first item for the chunk of lc taps from t0, of a tile whose first frame is f0
constexpr uint64_t extract_stage_base(uint64_t L, uint64_t D, uint64_t f0, uint64_t t0, uint64_t lc)
{
    return (L - 1) + f0 * D + (D - 1) - (t0 + lc - 1); // t0 + lc <= L: the difference is taken last, nothing goes negative
}
// items of that stage for the tile's nv >= 1 frames that lie inside the span
constexpr uint64_t extract_stage_items(uint64_t D, uint64_t nv, uint64_t lc) { return (nv - 1) * D + lc; }
// frames of the tile at column c0 that lie inside a span of n_frames: 0 .. T
constexpr unsigned extract_tile_frames(uint64_t c0, unsigned n_frames, unsigned T)
{
    return c0 >= n_frames ? 0u : n_frames - c0 < T ? static_cast<unsigned>(n_frames - c0) : T;
}
constexpr bool extract_in_buffer(uint64_t u, uint64_t lo, uint64_t hi) { return u >= lo && u < hi; }

// whether the frames [first_frame, first_frame + n_frames) keep every index below 2^64 - 1: the absolute index of the
// newest sample, and the kernel's
constexpr bool extract_span_fits(uint64_t first_frame, uint64_t n_frames, uint64_t D, uint64_t L, uint64_t start_index)
{
    if (first_frame > UINT64_MAX - n_frames) return false;
    const uint64_t end = first_frame + n_frames;
    if (end > UINT64_MAX / D) return false;
    const uint64_t most = start_index > L - 1 ? start_index : L - 1;
    return end * D <= UINT64_MAX - 1 - most;
}

inline ExtractPlan extract_plan(size_t I, size_t K, size_t D, size_t L, unsigned T, uint64_t start_index, bool have_in,
                                size_t n_in, uint64_t in_index, const ExtractSpan* spans, size_t n_spans, bool have_out,
                                size_t out_stride, size_t n_cols)
{
    ExtractPlan p = {ExtractRefusal::none, 0, 0, 0, 0, 0, 0};
    auto refuse = [&](ExtractRefusal why, size_t at) {
        p.why = why, p.at = at;
        return p;
    };
    if (I > 1) return refuse(ExtractRefusal::rational, 0);
    if (n_spans == 0 || n_cols == 0) return refuse(ExtractRefusal::nothing, 0);
    if (n_spans > kMaxExtractSpans || !spans) return refuse(ExtractRefusal::spans, 0);
    for (size_t b = 0; b < n_spans; ++b) {
        if (spans[b].channel >= K) return refuse(ExtractRefusal::channel, b);
        if (spans[b].n_frames > n_cols) return refuse(ExtractRefusal::room, b);
        if (!extract_span_fits(spans[b].first_frame, spans[b].n_frames, D, L, start_index))
            return refuse(ExtractRefusal::overflow, b);
    }
    if (n_spans > 1 && out_stride < n_cols) return refuse(ExtractRefusal::stride, 0);
    if (!have_out) return refuse(ExtractRefusal::output, 0);
    if (n_in && !have_in) return refuse(ExtractRefusal::input, 0);
    if (in_index > UINT64_MAX - n_in) return refuse(ExtractRefusal::overflow, n_spans);
    const uint64_t tiles = (static_cast<uint64_t>(n_cols) + T - 1) / T;
    if (tiles > 0x7FFFFFFFu) return refuse(ExtractRefusal::overflow, n_spans);
    p.grid_x = static_cast<unsigned>(tiles);
    p.grid_y = static_cast<unsigned>(n_spans);
    // the buffer, less what lies before the handle's start; a buffer that begins beyond every index a span may reach
    // (2^64 - 2) is as good as none
    const uint64_t end = in_index + n_in, first = in_index > start_index ? in_index : start_index;
    if (end > first && first - start_index <= UINT64_MAX - (L - 1)) {
        p.lo = first - start_index + (L - 1);
        p.hi = end - start_index > UINT64_MAX - (L - 1) ? UINT64_MAX : end - start_index + (L - 1);
        p.skip = first - in_index;
    }
    return p;
}

struct BurstSpan {
    uint64_t first_frame, n_frames; // n_frames may exceed a span's 32 bits: the caller splits or refuses
};

// the frames that see the samples [start_sample, end_sample) of the wideband stream, widened by `margin` frames on
// either side: from max(0, floor((start_sample - start_index) / D) - margin), the first frame whose newest sample is
// at or after start_sample, to ceil((end_sample - start_index + L - 1) / D) + margin, a frame whose oldest sample is
// at or after end_sample.  Both are clamped to the frames extract_span_fits() admits; an empty burst gives no frame.
inline BurstSpan burst_span(uint64_t start_sample, uint64_t end_sample, uint64_t D, uint64_t L, uint64_t start_index,
                            uint64_t margin)
{
    if (end_sample <= start_sample) return BurstSpan{0, 0};
    const uint64_t most = start_index > L - 1 ? start_index : L - 1;
    if ((UINT64_MAX - 1 - most) / D < 1) return BurstSpan{0, 0};
    const uint64_t last_most = (UINT64_MAX - 1 - most) / D - 1; // (last_most + 1) D + most <= 2^64 - 2
    const uint64_t q = start_sample > start_index ? (start_sample - start_index) / D : 0;
    uint64_t first = q > margin ? q - margin : 0;
    // end_sample - start_index + L - 1, not below 0 and saturating
    uint64_t num = 0;
    if (end_sample >= start_index)
        num = end_sample - start_index > UINT64_MAX - (L - 1) ? UINT64_MAX : end_sample - start_index + (L - 1);
    else if (start_index - end_sample < L - 1)
        num = (L - 1) - (start_index - end_sample);
    uint64_t last = num / D + (num % D ? 1 : 0);
    last = last > UINT64_MAX - margin ? UINT64_MAX : last + margin;
    if (last > last_most) last = last_most;
    if (first > last) first = last;
    return BurstSpan{first, last - first + 1};
}

} // namespace hostlogic
} // namespace gr4pm
