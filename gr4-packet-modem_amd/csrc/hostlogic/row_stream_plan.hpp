// hostlogic/row_stream_plan.hpp -- the host side of gr4pm_row_stream (csrc/row_stream.hip), HIP-free:
// a row's carried state and its advance over a call, the count of a call and of a flush, the rebase of the phase
// reference, set_row, the first item behind start_index, the call's validation and the launch geometry.  The branch,
// alpha, theta, the tile and the span bound are hostlogic/row_resample_plan.hpp's; the kernel uses these very
// expressions, and tests/hostlogic/row_stream_plan_check.cpp sweeps them against __int128 restatements.
//
// Positions.  pos_m = phase0 + m step is unbounded (start_index may be 2^63, and a stream has no end), so no absolute
// position is kept.  A row keeps A, the absolute index of the next input item, and d = pos_next - A 2^32 for its next
// output item.  Every item with floor(pos) <= A - 1 has been made, so d >= 0; d < 2^63 at create (d < step, or d =
// phase0 - start 2^32 <= phase0) and never grows.  A call of n items makes the k >= 0 with d + k step < n 2^32 and the
// kernel works with d + k step: n + P - 1 < 2^32 keeps that, and it plus (P - 1) 2^32 (the stage's origin is A - (P - 1),
// the first history item), below 2^64.
// Phase.  theta(pos) = Phi + floor(freq (pos - ref) / 2^32) mod 2^32.  Moving ref by B whole items and adding freq B to
// Phi changes no theta, so ref is kept at (A - 1) 2^32 + ref_frac, ref_frac < 2^32: one item in front of every position
// a call can make, whatever P is.  The kernel's operand is d + k step + 2^32 - ref_frac, positive and below 2^64.
#pragma once
#include "row_resample_plan.hpp"

namespace gr4pm {
namespace hostlogic {

struct RowStreamRow {
    uint64_t step, phase0, start; // the record's and start_index; step is the current one (set_row)
    int32_t freq;                 // the current one
    uint32_t phi;                 // Phi for ref = (items_in - 1) 2^32 + ref_frac
    uint32_t ref_frac;
    uint32_t hist;                // which of the two history buffers holds the row's last P - 1 items
    uint64_t items_in;            // A
    uint64_t items_out;           // the index of the next output item, mod 2^64
    uint64_t d;                   // its position minus A 2^32, Q32.32
};

// (hi 2^32 + lo) / step for step < 2^39: the quotient mod 2^64 and the remainder, 16 bits of the dividend at a time so
// that no partial dividend leaves 64 bits
struct RowDiv {
    uint64_t quot, rem;
};
constexpr RowDiv row_div96(uint64_t hi, uint32_t lo, uint64_t step)
{
    uint64_t q = hi / step, r = hi % step; // r < 2^39
    for (int part = 1; part >= 0; --part) {
        const uint64_t v = (r << 16) | ((lo >> (16 * part)) & 0xffffu); // below 2^55
        q = (q << 16) + v / step; // v / step < 2^16: r < step
        r = v % step;
    }
    return RowDiv{q, r};
}

// the created state for the row's step, phase0, start and freq: the first m with floor(pos_m) >= start, Phi = 0 and
// ref = 0 (moved to item start - 1).  The history is +0: the caller clears the device's.
constexpr void row_stream_start(RowStreamRow& s)
{
    s.items_in = s.start;
    s.ref_frac = 0;
    s.phi = static_cast<uint32_t>(s.freq) * static_cast<uint32_t>(s.start - 1); // wraps as it must for start = 0
    if ((s.phase0 >> 32) >= s.start) {
        s.items_out = 0;
        s.d = s.phase0 - (s.start << 32); // start <= phase0 >> 32 < 2^31
        return;
    }
    // N = start 2^32 - phase0 > 0, up to 96 bits; m = ceil(N / step), d = m step - N
    const uint32_t pl = static_cast<uint32_t>(s.phase0);
    const uint32_t lo = 0u - pl;
    const uint64_t hi = s.start - (s.phase0 >> 32) - (pl != 0 ? 1 : 0);
    const RowDiv q = row_div96(hi, lo, s.step);
    s.items_out = q.quot + (q.rem != 0 ? 1 : 0);
    s.d = q.rem != 0 ? s.step - q.rem : 0;
}

// the items a row makes over `span` further input items, span < 2^32: the k >= 0 with d + k step < span 2^32
constexpr uint64_t row_stream_count(const RowStreamRow& s, uint64_t span)
{
    const uint64_t end = span << 32;
    return s.d >= end ? 0 : (end - 1 - s.d) / s.step + 1;
}
// what a flush makes: the filter runs out over P - 1 items of +0
constexpr uint64_t row_stream_flush_count(const RowStreamRow& s, uint64_t P) { return row_stream_count(s, P - 1); }

// the state behind a call that took n items and made count = row_stream_count(s, n) of them; kept a buffer flip aside
constexpr void row_stream_advance(RowStreamRow& s, uint64_t n, uint64_t count)
{
    const uint64_t end = n << 32;
    if (count == 0) {
        s.d -= end;
    } else {
        const uint64_t last = s.d + (count - 1) * s.step; // < end
        s.d = s.step - (end - last);                      // last + step >= end
    }
    s.items_in += n;
    s.items_out += count;
    s.phi += static_cast<uint32_t>(s.freq) * static_cast<uint32_t>(n); // ref moves n items with A
    if (n != 0) s.hist ^= 1u;
}

// the kernel's operand of row_theta for the item at d + k step =: rel
constexpr uint64_t row_stream_theta_pos(uint64_t rel, uint32_t ref_frac) { return rel + (uint64_t(1) << 32) - ref_frac; }
constexpr uint32_t row_stream_theta(const RowStreamRow& s, uint64_t rel)
{
    return s.phi + row_theta(s.freq, row_stream_theta_pos(rel, s.ref_frac));
}

// set_row: the next item's position p* = A 2^32 + d stays, Phi <- theta_old(p*), ref <- p*, which is then moved back by
// (d >> 32) + 1 items to item A - 1
constexpr void row_stream_retune(RowStreamRow& s, uint64_t step, int32_t freq)
{
    const uint32_t at = row_stream_theta(s, s.d);
    s.step = step, s.freq = freq;
    s.ref_frac = static_cast<uint32_t>(s.d);
    s.phi = at - static_cast<uint32_t>(freq) * static_cast<uint32_t>((s.d >> 32) + 1);
}

// of RowRefusal a stream's call has none, length, items, columns, stride, lengths, room, output (no output array although
// there are columns) and input
using RowStreamRefusal = RowRefusal;

struct RowStreamPlan {
    RowStreamRefusal why;
    size_t at;
    uint32_t T;              // output items of a tile
    uint32_t grid_x, grid_y; // tiles (0: no column), rows
    uint32_t n[kRowMaxRows]; // the rows' input items of this call (0 in a flush)
    uint32_t M[kRowMaxRows]; // the rows' output items of this call
};

// validates process (flush = false) or flush (flush = true: x, stride, n_cols and lengths are not looked at) and gives
// the counts and the grid; changes nothing
inline RowStreamPlan row_stream_plan(const RowStreamRow* rows, size_t n_rows, uint64_t P, bool flush, bool have_x, size_t stride,
                                     size_t n_cols, const uint64_t* lengths, bool have_out, size_t out_stride, uint64_t n_cols_out,
                                     bool have_out_lengths)
{
    RowStreamPlan p = {};
    auto refuse = [&](RowStreamRefusal why, size_t at) {
        p.why = why, p.at = at;
        return p;
    };
    bool any = false;
    uint64_t max_step = 0;
    for (size_t r = 0; r < n_rows; ++r) {
        const uint64_t n = flush ? 0 : lengths ? lengths[r] : n_cols;
        if (n > n_cols && !flush) return refuse(RowStreamRefusal::length, r);
        if (!row_stream_items_valid(n, P)) return refuse(RowStreamRefusal::items, r);
        p.n[r] = static_cast<uint32_t>(n);
        any = any || n != 0;
        if (rows[r].step > max_step) max_step = rows[r].step;
    }
    if (n_cols_out > kRowMaxColsOut) return refuse(RowStreamRefusal::columns, 0);
    if (n_rows > 1 && ((!flush && stride < n_cols) || out_stride < n_cols_out)) return refuse(RowStreamRefusal::stride, 0);
    if (!have_out_lengths) return refuse(RowStreamRefusal::lengths, 0);
    for (size_t r = 0; r < n_rows; ++r) {
        const uint64_t M = flush ? row_stream_flush_count(rows[r], P) : row_stream_count(rows[r], p.n[r]);
        if (M > n_cols_out) return refuse(RowStreamRefusal::room, r);
        p.M[r] = static_cast<uint32_t>(M);
    }
    if (n_cols_out != 0 && !have_out) return refuse(RowStreamRefusal::output, 0);
    if (any && !have_x) return refuse(RowStreamRefusal::input, 0);
    p.T = row_tile(P, max_step);
    p.grid_x = static_cast<uint32_t>((n_cols_out + p.T - 1) / p.T);
    p.grid_y = static_cast<uint32_t>(n_rows);
    return p;
}

// the stage of a tile: item j is the row's item A - (P - 1) + i0 + j for the tile's first i0 = (d + m0 step) >> 32.
// k = i0 - (P - 1) + j is its index relative to A: below 0 it is history item (P - 1) + k (+0, and not loaded, in a
// one-shot call: a fresh row's history), in [0, n) it is x[k], and at or behind n it is +0 and not loaded (of a stream
// only a flush reaches those)
enum class RowStreamSource { history, input, zero };
constexpr RowStreamSource row_stream_source(int64_t k, uint64_t n)
{
    return row_item_loaded(k, n) ? RowStreamSource::input : k < 0 ? RowStreamSource::history : RowStreamSource::zero;
}

// the keep kernel: new history item j of a row that took n > 0 items is the item at k = n - (P - 1) + j relative to A
constexpr int64_t row_stream_keep_index(uint64_t n, uint64_t P, uint64_t j)
{
    return static_cast<int64_t>(n) - static_cast<int64_t>(P - 1) + static_cast<int64_t>(j);
}

} // namespace hostlogic
} // namespace gr4pm
