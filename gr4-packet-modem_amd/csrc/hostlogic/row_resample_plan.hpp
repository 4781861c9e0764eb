// hostlogic/row_resample_plan.hpp -- the host side of gr4pm_row_resampler (csrc/row_resampler.hip, DESIGN.md section
// 24), HIP-free: the position arithmetic of an output item, a row's output length, the tile the host picks for a call,
// the index test the kernel stages by, and one function that validates a call.  The kernel uses these very expressions;
// tests/hostlogic/row_resample_plan_check.cpp sweeps them against __int128 restatements.
//
// Positions.  Output item m of a row has pos = phase0 + m step in input items with 32 fractional bits: i = pos >> 32 is
// the newest input item it takes (tap s from item i - s), mu = pos & 0xffffffff the fraction the coefficients are
// interpolated at.  A row of n items has the items m with i <= n + P - 2, so pos < (n + P - 1) 2^32 =: E; the plan refuses
// n + P - 1 >= 2^32 and phase0 >= 2^63, so E fits 64 bits and no position of an item that exists wraps.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../../include/gr4pm_hip.h"

namespace gr4pm {
namespace hostlogic {

using RowRecord = gr4pm_row_record; // step, phase0, freq

constexpr size_t kRowMaxRows = 64;        // of a call: the records travel by value
constexpr size_t kRowMaxTaps = 4096;      // Q P
constexpr uint32_t kRowMinPhases = 2, kRowMaxPhases = 256;
constexpr uint32_t kRowStageItems = 4096; // complex64 input items of a tile in LDS: 32 KiB beside at most 32 KiB of tables
constexpr uint32_t kRowThreads = 256;
constexpr uint32_t kRowMaxTile = 1024;    // output items of a tile: four per thread
constexpr uint64_t kRowMinStep = uint64_t(1) << 26, kRowMaxStep = uint64_t(1) << 38;
constexpr uint64_t kRowMaxColsOut = uint64_t(1) << 31;

constexpr bool row_phases_valid(uint64_t Q) { return Q >= kRowMinPhases && Q <= kRowMaxPhases && (Q & (Q - 1)) == 0; }
constexpr bool row_sizes_valid(uint64_t Q, uint64_t P) { return row_phases_valid(Q) && P >= 1 && P <= kRowMaxTaps / Q; }
constexpr uint32_t row_log2(uint32_t Q)
{
    uint32_t l = 0;
    while ((uint32_t(1) << l) < Q) ++l;
    return l;
}
constexpr bool row_step_valid(uint64_t step) { return step >= kRowMinStep && step <= kRowMaxStep; }
// a row of n items, or a call that brings a carried row n more: n + P - 1 < 2^32
constexpr bool row_stream_items_valid(uint64_t n, uint64_t P) { return n <= UINT64_MAX - (P - 1) && n + (P - 1) < (uint64_t(1) << 32); }

// the branch q and the numerator of alpha for the fraction mu with b = 32 - log2 Q
constexpr uint32_t row_branch(uint32_t mu, uint32_t b) { return mu >> b; }
constexpr uint32_t row_alpha_bits(uint32_t mu, uint32_t b) { return mu & ((uint32_t(1) << b) - 1u); }

// floor(freq pos / 2^32) mod 2^32 for the signed word: the integer part wraps, the fraction's product is shifted
// arithmetically
constexpr uint32_t row_theta(int32_t freq, uint64_t pos)
{
    const uint32_t hi = static_cast<uint32_t>(freq) * static_cast<uint32_t>(pos >> 32);
    const int64_t prod = static_cast<int64_t>(freq) * static_cast<int64_t>(pos & 0xffffffffu);
    return hi + static_cast<uint32_t>(static_cast<uint64_t>(prod >> 32));
}

// items of a row of n input items, before the cut at the output's columns: the m with phase0 + m step < (n + P - 1) 2^32.
// The caller has checked n + P - 1 < 2^32, phase0 < 2^63 and the step's range.
constexpr uint64_t row_output_items(uint64_t n, uint64_t P, uint64_t step, uint64_t phase0)
{
    if (n == 0) return 0;
    const uint64_t end = (n + P - 1) << 32;
    return phase0 >= end ? 0 : (end - 1 - phase0) / step + 1;
}

// input items a tile of t output items can span at `step`, whatever its first position: floor(pos + (t - 1) step) -
// floor(pos) <= ceil((t - 1) step), plus the P items the first one takes
constexpr uint64_t row_span_bound(uint64_t t, uint64_t step, uint64_t P) { return (((t - 1) * step + 0xffffffffu) >> 32) + P; }

// the tile of a call whose largest step is max_step: the most items, up to kRowMaxTile, whose span fits the stage, cut to
// a multiple of the workgroup (or of a wave) where it exceeds one; at least 1, since P <= kRowMaxTaps / 2 < the stage
constexpr uint32_t row_tile(uint64_t P, uint64_t max_step)
{
    const uint64_t room = (static_cast<uint64_t>(kRowStageItems) - P) << 32; // (t - 1) step <= room
    uint64_t t = 1 + room / max_step;
    if (t > kRowMaxTile) t = kRowMaxTile;
    if (t >= kRowThreads)
        t -= t % kRowThreads;
    else if (t >= 64)
        t -= t % 64;
    return static_cast<uint32_t>(t);
}

// items of the tile at column m0 that lie below a row's M items: 0 .. T
constexpr uint32_t row_tile_items(uint64_t m0, uint64_t M, uint32_t T)
{
    return m0 >= M ? 0u : M - m0 < T ? static_cast<uint32_t>(M - m0) : T;
}
// the input items the tile's nv >= 1 items take, from item (pos0 >> 32) - (P - 1) on
constexpr uint64_t row_tile_span(uint64_t pos0, uint32_t nv, uint64_t step, uint64_t P)
{
    return ((pos0 + static_cast<uint64_t>(nv - 1) * step) >> 32) - (pos0 >> 32) + P;
}
// whether input index k of a row of n items exists: every other one is the operand +0 and is not loaded
constexpr bool row_item_loaded(int64_t k, uint64_t n) { return k >= 0 && static_cast<uint64_t>(k) < n; }

enum class RowRefusal { // of a one-shot call (row_plan) and of a stream's (row_stream_plan.hpp)
    none,     // launch
    nothing,  // no row or no column: OK, nothing to launch (out_lengths are written when there are rows)
    rows,     // more than kRowMaxRows
    records,  // no record array
    length,   // lengths[at] > n_cols
    step,     // rows[at].step out of range
    items,    // lengths[at] + P - 1 >= 2^32
    phase,    // rows[at].phase0 >= 2^63
    columns,  // n_cols_out > 2^31
    stride,   // R > 1 with a stride below the column count, on either side
    lengths,  // no out_lengths array
    room,     // a stream's row `at` makes more than n_cols_out items in this call: a stream loses none, so nothing is cut
    output,   // no output array
    input,    // no input array although a row has items
};

struct RowPlan {
    RowRefusal why;
    size_t at;               // the row a refusal names
    uint32_t T;              // output items of a tile
    uint32_t grid_x, grid_y; // tiles, rows
    uint32_t n[kRowMaxRows]; // the rows' input items
    uint32_t M[kRowMaxRows]; // the rows' output items, cut at n_cols_out
};

inline RowPlan row_plan(uint64_t P, bool have_x, size_t stride, size_t n_cols, const uint64_t* lengths, const RowRecord* rows,
                        size_t n_rows, bool have_out, size_t out_stride, uint64_t n_cols_out, bool have_out_lengths)
{
    RowPlan p = {};
    auto refuse = [&](RowRefusal why, size_t at) {
        p.why = why, p.at = at;
        return p;
    };
    if (n_rows > kRowMaxRows) return refuse(RowRefusal::rows, 0);
    if (n_rows == 0) return refuse(RowRefusal::nothing, 0);
    if (!rows) return refuse(RowRefusal::records, 0);
    if (n_cols_out > kRowMaxColsOut) return refuse(RowRefusal::columns, 0);
    bool any = false;
    uint64_t max_step = 0;
    for (size_t r = 0; r < n_rows; ++r) {
        const uint64_t n = lengths ? lengths[r] : n_cols;
        if (n > n_cols) return refuse(RowRefusal::length, r);
        if (!row_step_valid(rows[r].step)) return refuse(RowRefusal::step, r);
        if (!row_stream_items_valid(n, P)) return refuse(RowRefusal::items, r);
        if (rows[r].phase0 >= (uint64_t(1) << 63)) return refuse(RowRefusal::phase, r);
        const uint64_t M = row_output_items(n, P, rows[r].step, rows[r].phase0);
        p.n[r] = static_cast<uint32_t>(n);
        p.M[r] = static_cast<uint32_t>(M < n_cols_out ? M : n_cols_out);
        any = any || n != 0;
        if (rows[r].step > max_step) max_step = rows[r].step;
    }
    if (n_rows > 1 && (stride < n_cols || out_stride < n_cols_out)) return refuse(RowRefusal::stride, 0);
    if (!have_out_lengths) return refuse(RowRefusal::lengths, 0);
    if (n_cols_out == 0) return refuse(RowRefusal::nothing, 0);
    if (!have_out) return refuse(RowRefusal::output, 0);
    if (any && !have_x) return refuse(RowRefusal::input, 0);
    p.T = row_tile(P, max_step);
    p.grid_x = static_cast<uint32_t>((n_cols_out + p.T - 1) / p.T);
    p.grid_y = static_cast<uint32_t>(n_rows);
    return p;
}

} // namespace hostlogic
} // namespace gr4pm
