// hostlogic/row_gate_plan.hpp -- the host side of gr4pm_row_gate (csrc/row_gate.hip), HIP-free: a
// row's carried state, the step of its state machine over the block sums of a call, the flush, the record of a span,
// what the device retains, the refusals and the plan of a whole call on copies of the rows, so that a refused call
// (capacity included) has touched nothing.  tests/hostlogic/row_gate_plan_check.cpp sweeps it against a restatement that
// sees all block sums of a row at once.
//
// Positions.  A row counts items and blocks from 0 in uint64.  Only block indices are kept (first_active, last_active,
// start, keep_first, decided); an item position is block * B with block <= items / B, so no product leaves 64 bits while
// the item count itself fits them.  What a kernel is handed is relative to the call's first new item: a signed 64-bit k
// with -retained <= k < n, retained <= (max_blocks + 1) B - 1 and n < 2^32 - max_blocks B.
// Retained items.  The device keeps the row's items from block keep_first on: the open span from `start` while a burst
// is open (fewer than max_blocks blocks: the block that completes max_blocks ends the burst), the last pre_blocks decided
// blocks while idle, and the items of the incomplete block behind them: at most (max_blocks + 1) B - 1 items.
#pragma once
#include <cstddef>
#include <cstdint>

namespace gr4pm {
namespace hostlogic {

constexpr size_t kRowGateMaxRows = 64;
constexpr uint32_t kRowGateMinBlock = 16, kRowGateMaxBlock = 1024;
constexpr uint64_t kRowGateMaxCols = uint64_t(1) << 30;
constexpr uint32_t kRowGateTruncated = 1u; // the span ends at the block that completed max_blocks; the burst went on
constexpr uint32_t kRowGateAtEnd = 2u;     // closed by flush: the row ended while the burst was open

struct RowGateParams {
    uint32_t B, hold, min_blocks, pre, post, max_blocks;
};

enum class RowGateRefusal {
    none,
    rows,       // R outside 1 .. 64
    block,      // B no power of two in [16, 1024]
    min_blocks, // min_blocks = 0
    hold,       // hold_blocks >= 2^31
    post,       // post_blocks > hold_blocks + 1
    budget,     // pre_blocks + min_blocks + post_blocks > max_blocks
    columns,    // max_blocks B > n_cols, or n_cols > 2^30
    pointer,    // an array that is needed is NULL
    length,     // lengths[at] > stride
    items,      // lengths[at] >= 2^32 - max_blocks B
    thresholds, // not 0 < close_sum <= open_sum (NaN included)
    capacity,   // the call emits more bursts than `cap`
};

constexpr RowGateRefusal row_gate_params_check(uint64_t R, const RowGateParams& p, uint64_t n_cols)
{
    if (R < 1 || R > kRowGateMaxRows) return RowGateRefusal::rows;
    if (p.B < kRowGateMinBlock || p.B > kRowGateMaxBlock || (p.B & (p.B - 1)) != 0) return RowGateRefusal::block;
    if (p.min_blocks < 1) return RowGateRefusal::min_blocks;
    if (p.hold >= (uint32_t(1) << 31)) return RowGateRefusal::hold;
    if (uint64_t(p.post) > uint64_t(p.hold) + 1) return RowGateRefusal::post;
    if (uint64_t(p.pre) + p.min_blocks + p.post > p.max_blocks) return RowGateRefusal::budget;
    if (n_cols > kRowGateMaxCols || uint64_t(p.max_blocks) * p.B > n_cols) return RowGateRefusal::columns;
    return RowGateRefusal::none;
}
constexpr bool row_gate_thresholds_valid(float open_sum, float close_sum) { return 0.0f < close_sum && close_sum <= open_sum; }
constexpr bool row_gate_length_valid(uint64_t n, const RowGateParams& p)
{
    return n < (uint64_t(1) << 32) - uint64_t(p.max_blocks) * p.B;
}

struct RowGateRow {
    uint64_t items, decided;                    // items taken, blocks decided
    uint64_t first_active, last_active, start;  // of the open burst (blocks)
    uint64_t keep_first;                        // the first block the device still retains
    uint64_t emitted, dropped, truncated;       // bursts, since create / reset / flush
    double sum;                                 // of the open burst's active blocks, in block order
    float peak;                                 // the largest of them
    float open_sum, close_sum;                  // what the next block decided is compared against
    uint32_t run;                               // inactive blocks in a row behind last_active
    uint32_t open;                              // 1: a burst is open
    uint32_t hist;                              // which of the two history buffers holds the retained items
};

// the created state; the thresholds stay
constexpr void row_gate_start(RowGateRow& s)
{
    const float o = s.open_sum, c = s.close_sum;
    s = RowGateRow{};
    s.open_sum = o, s.close_sum = c;
}

constexpr uint64_t row_gate_partial(const RowGateRow& s, uint32_t B) { return s.items - s.decided * B; }   // < B
constexpr uint64_t row_gate_retained(const RowGateRow& s, uint32_t B) { return s.items - s.keep_first * B; }
// the blocks that n further items complete
constexpr uint64_t row_gate_blocks_for(const RowGateRow& s, uint32_t B, uint64_t n) { return (row_gate_partial(s, B) + n) / B; }
constexpr uint64_t row_gate_retained_bound(const RowGateParams& p) { return (uint64_t(p.max_blocks) + 1) * p.B - 1; }

struct RowGateSpan {
    uint64_t start, end; // blocks, both inclusive
    uint64_t first_active, last_active;
    double sum;
    float peak;
    uint32_t flags;
};

// Decides the row's next n_blocks blocks, whose sums are sums[0 .. n_blocks).  Returns how many spans they emit and
// writes the first min(that, cap) of them to out.  Per block c:
//   idle: sums >= open_sum opens (first_active = last_active = c, start = max(0, c - pre)); anything else stays idle
//   open: sums >= close_sum is active (last_active = c), anything else (a NaN too) extends the inactive run, and the
//         run's block hold + 1 closes: dropped below min_blocks, else the span [start, last_active + post]
//   still open behind that, and c - start + 1 == max_blocks: the span [start, c] with kRowGateTruncated; idle
inline size_t row_gate_step(RowGateRow& s, const RowGateParams& p, const float* sums, size_t n_blocks, RowGateSpan* out, size_t cap)
{
    size_t count = 0;
    auto emit = [&](uint64_t end, uint32_t flags) {
        if (count < cap) out[count] = RowGateSpan{s.start, end, s.first_active, s.last_active, s.sum, s.peak, flags};
        ++count;
        ++s.emitted;
        if (flags & kRowGateTruncated) ++s.truncated;
        s.open = 0;
    };
    for (size_t j = 0; j < n_blocks; ++j, ++s.decided) {
        if (!s.open) { // silence is most of a stream: over it nothing but the comparison
            const float open_sum = s.open_sum;
            size_t k = j;
            while (k < n_blocks && !(sums[k] >= open_sum)) ++k;
            s.decided += k - j, j = k;
            if (j == n_blocks) break;
        }
        const uint64_t c = s.decided;
        const float v = sums[j];
        if (!s.open) {
            if (!(v >= s.open_sum)) continue;
            s.open = 1, s.run = 0;
            s.first_active = s.last_active = c;
            s.start = c > p.pre ? c - p.pre : 0;
            s.sum = static_cast<double>(v), s.peak = v;
        } else if (v >= s.close_sum) {
            s.last_active = c, s.run = 0;
            s.sum += static_cast<double>(v);
            if (v > s.peak) s.peak = v;
        } else if (++s.run == p.hold + 1) {
            if (s.last_active - s.first_active + 1 < p.min_blocks) {
                ++s.dropped;
                s.open = 0;
            } else {
                emit(s.last_active + p.post, 0); // <= c: post <= hold + 1
            }
            continue;
        }
        if (c - s.start + 1 == p.max_blocks) emit(c, kRowGateTruncated);
    }
    return count;
}

// the end of the row: the block the partial items make with +0 behind them (partial_sum, or NULL when the row ends on
// a block edge), then inactive blocks without end: an open burst closes at once, its post margin clipped to the
// blocks that exist.  The caller restores the created state behind it.
inline size_t row_gate_finish(RowGateRow& s, const RowGateParams& p, const float* partial_sum, RowGateSpan* out, size_t cap)
{
    size_t count = row_gate_step(s, p, partial_sum, partial_sum ? 1 : 0, out, cap);
    if (!s.open) return count;
    s.open = 0;
    if (s.last_active - s.first_active + 1 < p.min_blocks) {
        ++s.dropped;
        return count;
    }
    const uint64_t want = s.last_active + p.post, last = s.decided - 1;
    if (count < cap) out[count] = RowGateSpan{s.start, want < last ? want : last, s.first_active, s.last_active, s.sum, s.peak, kRowGateAtEnd};
    ++s.emitted;
    return count + 1;
}

// behind a step that took n items: the count, and what the device retains from here on
constexpr void row_gate_take(RowGateRow& s, const RowGateParams& p, uint64_t n)
{
    s.items += n;
    s.keep_first = s.open ? s.start : (s.decided > p.pre ? s.decided - p.pre : 0);
    if (n != 0) s.hist ^= 1u;
}

struct RowGateRecord {
    uint64_t first_item, first_active_item;
    double power;
    uint32_t n_items, active_items, flags;
    float peak;
};
// items: the row's items at the end of the call: only a flush has spans and active extents that reach behind them
constexpr RowGateRecord row_gate_record(const RowGateSpan& sp, uint32_t B, uint64_t items)
{
    const uint64_t first = sp.start * B, fa = sp.first_active * B;
    const uint64_t end = (sp.end + 1) * B < items ? (sp.end + 1) * B : items;
    const uint64_t active_end = (sp.last_active + 1) * B < items ? (sp.last_active + 1) * B : items;
    RowGateRecord r = {};
    r.first_item = first, r.first_active_item = fa;
    r.n_items = static_cast<uint32_t>(end - first);
    r.active_items = static_cast<uint32_t>(active_end - fa);
    r.power = sp.sum / static_cast<double>(r.active_items);
    r.flags = sp.flags, r.peak = sp.peak;
    return r;
}

// validates the arrays and lengths of a process call; changes nothing
inline RowGateRefusal row_gate_call_check(const RowGateParams& p, size_t R, bool have_x, uint64_t stride, const uint64_t* lengths,
                                          bool have_out, bool have_records, bool have_count, size_t cap, size_t* at)
{
    *at = 0;
    if (!lengths || !have_count || (cap != 0 && (!have_out || !have_records))) return RowGateRefusal::pointer;
    bool any = false;
    for (size_t r = 0; r < R; ++r) {
        *at = r;
        if (lengths[r] > stride) return RowGateRefusal::length;
        if (!row_gate_length_valid(lengths[r], p)) return RowGateRefusal::items;
        any = any || lengths[r] != 0;
    }
    *at = 0;
    if (any && !have_x) return RowGateRefusal::pointer;
    return RowGateRefusal::none;
}

// The plan of a call, on copies: next[r] becomes rows[r] behind the call, rows is not written.  sums + offs[r]: the
// n_blocks[r] block sums of row r (flush: n_blocks[r] is 0 or 1, the zero-completed partial block).  Spans go to out in
// the order (row, time), their rows to span_row, the first `cap` of them; returns the count.  The caller commits (rows
// <- next) only when the count is at most cap: a capacity refusal has moved nothing.
inline size_t row_gate_plan_call(const RowGateRow* rows, RowGateRow* next, size_t R, const RowGateParams& p, const float* sums,
                                 const uint64_t* offs, const uint32_t* n_blocks, const uint64_t* lengths, bool flush,
                                 RowGateSpan* out, uint32_t* span_row, size_t cap)
{
    size_t count = 0;
    for (size_t r = 0; r < R; ++r) {
        next[r] = rows[r];
        const size_t room = count < cap ? cap - count : 0;
        RowGateSpan* dst = room ? out + count : nullptr;
        size_t got;
        if (flush) {
            got = row_gate_finish(next[r], p, n_blocks[r] ? sums + offs[r] : nullptr, dst, room);
        } else {
            got = row_gate_step(next[r], p, sums + offs[r], n_blocks[r], dst, room);
            row_gate_take(next[r], p, lengths[r]);
        }
        for (size_t i = 0; i < got && i < room; ++i) span_row[count + i] = static_cast<uint32_t>(r);
        count += got;
    }
    return count;
}

// the kernels' source of the item k items from the call's first new item (k < 0: retained; at or behind n: +0, which
// only a flush's zero-completed block reaches)
enum class RowGateSource { history, input, zero };
constexpr RowGateSource row_gate_source(int64_t k, uint64_t n)
{
    return k < 0 ? RowGateSource::history : static_cast<uint64_t>(k) < n ? RowGateSource::input : RowGateSource::zero;
}

// The block sum's order, fixed per B (the header states it): W = min(B, 64) lanes; lane l adds the powers of the
// block's items l, l + W, l + 2 W, ... in ascending order, starting from the first; then log2(W) folds, offsets W / 2
// down to 1: t[l] <- t[l] + t[l + offset] for l < offset.  The sum is t[0].  The kernel's wave works through 1024
// consecutive items of the call in 16 loads per lane: `per` loads make one lane sum, and a load holds 64 / W blocks.
constexpr uint32_t kRowGateWaveItems = 1024, kRowGateThreads = 256, kRowGateGroupItems = 4096;
constexpr uint32_t row_gate_lanes(uint32_t B) { return B < 64 ? B : 64; }
constexpr uint32_t row_gate_loads_per_block(uint32_t B) { return B < 64 ? 1 : B / 64; }

} // namespace hostlogic
} // namespace gr4pm
