// row_gate.hip -- the RowBurstGate: a power squelch on rows that carries its state from call to call and delivers every
// burst of every row once, as a zero-padded row of [bursts, n_cols].  Definition: include/gr4pm_hip.h, DESIGN.md section
// 30; the state machine, the records, what is retained and the refusals: hostlogic/row_gate_plan.hpp.
//
// k_row_gate_power: blockIdx.y is the row, blockIdx.x a group of 4096 items of the call's sequence (the row's retained
//   partial items, then x_r); each of the four waves works through 1024 of them in 16 loads of 8 bytes per lane, all
//   issued before the first sum.  A block's sum follows the order of the header: lane sums over `per` loads, then folds
//   over min(B, 64) lanes.  Items of blocks the call does not complete are not loaded; an index at or behind lengths[r]
//   is +0 by a range test (only flush's zero-completed block reaches those).  block_power is this kernel with nothing
//   retained and the caller's array as the destination.
// k_row_gate_gather: one workgroup per 1024 columns of an emitted burst row: the span's items from the retained items or
//   x_r, +0 behind n_items by a range test.
// k_row_gate_keep: one workgroup per row writes what the row retains from here on into the other of its two buffers
//   (source and destination overlap otherwise); a row without new items keeps its buffer.
// One stream, no atomics; per call one copy of the block sums to the host and one wait, in front of the plan.
// Built with EXACT_FLAGS; the power is written in __fmul_rn / __fadd_rn all the same.
#include "common.hpp"
#include "hostlogic/row_gate_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

using namespace gr4pm;
namespace hl = gr4pm::hostlogic;

struct GateRow { // 32 bytes
    uint64_t off;    // where the row's block sums go
    uint32_t n;      // new items of the call
    uint32_t keep;   // retained items in front of them
    uint32_t lead;   // the last `lead` of those are the incomplete block
    uint32_t blocks; // block sums of the call
    uint32_t hist;   // the buffer that holds the retained items
    uint32_t keep_new;
};

struct GateArgs {
    const float2* x;
    float2* hist; // [2][R][hist_items]
    float* sums;
    size_t stride;
    uint32_t B, R, hist_items;
    GateRow row[hl::kRowGateMaxRows];
};
static_assert(sizeof(GateArgs) <= 4096, "the argument block");

struct GateSpan { // an emitted burst row
    int64_t k0;   // its first item, relative to the call's first new item
    uint32_t n_items, row;
};

__device__ __forceinline__ const float2* history_of(const GateArgs& a, uint32_t buf, uint32_t r)
{
    return a.hist + (static_cast<size_t>(buf) * a.R + r) * a.hist_items;
}

// item k of the row relative to the call's first new item
__device__ __forceinline__ float2 item_at(const float2* __restrict__ hr, const float2* __restrict__ xr, int64_t k, uint32_t keep, uint32_t n)
{
    switch (hl::row_gate_source(k, n)) {
    case hl::RowGateSource::history: return hr[static_cast<int64_t>(keep) + k];
    case hl::RowGateSource::input: return xr[k];
    default: return float2{0.0f, 0.0f};
    }
}

__global__ __launch_bounds__(hl::kRowGateThreads) void k_row_gate_power(GateArgs a)
{
    constexpr uint32_t kLoads = hl::kRowGateWaveItems / 64;
    const uint32_t r = blockIdx.y, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const GateRow rec = a.row[r];
    const uint32_t B = a.B;
    // q counts the call's sequence: the `lead` retained items of the incomplete block, then the new ones
    const uint64_t q0 = (static_cast<uint64_t>(blockIdx.x) * 4 + wave) * hl::kRowGateWaveItems;
    const uint64_t q_end = static_cast<uint64_t>(rec.blocks) * B;
    if (q0 >= q_end) return;
    const float2* __restrict__ hr = history_of(a, rec.hist, r);
    const float2* __restrict__ xr = a.x + static_cast<size_t>(r) * a.stride;
    float p[kLoads];
#pragma unroll
    for (uint32_t t = 0; t < kLoads; ++t) {
        const uint64_t q = q0 + t * 64 + lane;
        float2 v = {0.0f, 0.0f};
        if (q < q_end) v = item_at(hr, xr, static_cast<int64_t>(q) - static_cast<int64_t>(rec.lead), rec.keep, rec.n);
        p[t] = __fadd_rn(__fmul_rn(v.x, v.x), __fmul_rn(v.y, v.y));
    }
    const uint32_t W = hl::row_gate_lanes(B), per = hl::row_gate_loads_per_block(B);
    const uint32_t first = static_cast<uint32_t>(q0 / B); // the first block of the wave: 1024 is a multiple of B
    float* __restrict__ dst = a.sums + rec.off;
    float acc = 0.0f;
#pragma unroll
    for (uint32_t t = 0; t < kLoads; ++t) {
        acc = (t % per == 0) ? p[t] : __fadd_rn(acc, p[t]);
        if ((t + 1) % per != 0) continue;
        float v = acc;
        for (uint32_t off = W >> 1; off != 0; off >>= 1) v = __fadd_rn(v, __shfl_down(v, off, W));
        // per >= 1 loads make one block of 64 lanes, or one load makes 64 / W blocks
        const uint32_t block = first + (t / per) * (64u / W) + lane / W;
        if (lane % W == 0 && block < rec.blocks) dst[block] = v;
    }
}

__global__ __launch_bounds__(hl::kRowGateThreads) void k_row_gate_gather(GateArgs a, const GateSpan* __restrict__ spans, float2* __restrict__ out,
                                                                         size_t out_stride, uint32_t n_cols, uint32_t tiles)
{
    const uint32_t i = blockIdx.x / tiles, c0 = (blockIdx.x % tiles) * 1024u;
    const GateSpan sp = spans[i];
    const GateRow rec = a.row[sp.row];
    const float2* __restrict__ hr = history_of(a, rec.hist, sp.row);
    const float2* __restrict__ xr = a.x + static_cast<size_t>(sp.row) * a.stride;
    float2* __restrict__ row = out + static_cast<size_t>(i) * out_stride;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t c = c0 + j * hl::kRowGateThreads + threadIdx.x;
        if (c >= n_cols) break;
        float2 v = {0.0f, 0.0f};
        if (c < sp.n_items) v = item_at(hr, xr, sp.k0 + c, rec.keep, rec.n);
        row[c] = v;
    }
}

__global__ __launch_bounds__(hl::kRowGateThreads) void k_row_gate_keep(GateArgs a)
{
    const uint32_t r = blockIdx.x;
    const GateRow rec = a.row[r];
    if (rec.n == 0) return; // the row keeps its buffer
    const float2* __restrict__ hr = history_of(a, rec.hist, r);
    float2* __restrict__ now = const_cast<float2*>(history_of(a, rec.hist ^ 1u, r));
    const float2* __restrict__ xr = a.x + static_cast<size_t>(r) * a.stride;
    const int64_t k0 = static_cast<int64_t>(rec.n) - static_cast<int64_t>(rec.keep_new); // >= -keep
    for (uint32_t j = threadIdx.x; j < rec.keep_new; j += hl::kRowGateThreads) now[j] = item_at(hr, xr, k0 + j, rec.keep, rec.n);
}

const char* refusal_text(hl::RowGateRefusal why)
{
    switch (why) {
    case hl::RowGateRefusal::rows: return "a handle has 1 .. 64 rows";
    case hl::RowGateRefusal::block: return "the block length is a power of two from 16 to 1024";
    case hl::RowGateRefusal::min_blocks: return "min_blocks is 1 or more";
    case hl::RowGateRefusal::hold: return "hold_blocks is 2^31 or more";
    case hl::RowGateRefusal::post: return "post_blocks exceeds hold_blocks + 1: the post margin would not have arrived at the closing block";
    case hl::RowGateRefusal::budget: return "pre_blocks + min_blocks + post_blocks exceeds max_blocks";
    case hl::RowGateRefusal::columns: return "max_blocks blocks do not fit n_cols, or n_cols exceeds 2^30";
    case hl::RowGateRefusal::pointer: return "an array that the call needs is NULL";
    case hl::RowGateRefusal::length: return "the row's length exceeds the stride";
    case hl::RowGateRefusal::items: return "the row's length reaches 2^32 - max_blocks * block";
    case hl::RowGateRefusal::thresholds: return "the sums need 0 < close_sum <= open_sum";
    case hl::RowGateRefusal::capacity: return "more bursts than the output has rows";
    default: return "";
    }
}

gr4pm_status refuse(hl::RowGateRefusal why, size_t at)
{
    if (why == hl::RowGateRefusal::none) return GR4PM_OK;
    set_error("row_gate: row %zu: %s", at, refusal_text(why));
    return why == hl::RowGateRefusal::items || why == hl::RowGateRefusal::capacity ? GR4PM_ERR_OVERFLOW : GR4PM_ERR_INVALID;
}

} // namespace

struct gr4pm_row_gate {
    hl::RowGateParams p = {};
    uint32_t R = 0, n_cols = 0, hist_items = 0;
    hipStream_t stream = nullptr;
    bool on_device = false; // the buffers are made by the first call that enqueues
    gr4pm::DevBuf<float2> d_hist;
    gr4pm::DevBuf<float> d_sums;
    gr4pm::DevBuf<GateSpan> d_spans;
    gr4pm::PinnedBuf<float> h_sums;
    std::vector<hl::RowGateRow> rows, next;
    std::vector<hl::RowGateSpan> spans;
    std::vector<uint32_t> span_row;
    std::vector<GateSpan> table;

    gr4pm_status device()
    {
        if (on_device) return GR4PM_OK;
        GR4PM_TRY(require_device());
        GR4PM_TRY(d_hist.alloc(2 * static_cast<size_t>(R) * hist_items));
        on_device = true;
        return GR4PM_OK;
    }

    void restart()
    {
        for (hl::RowGateRow& s : rows) hl::row_gate_start(s);
    }

    void base_args(GateArgs& a, const gr4pm_c64* x, size_t stride) const
    {
        a.x = reinterpret_cast<const float2*>(x), a.hist = d_hist.p, a.stride = stride;
        a.B = p.B, a.R = R, a.hist_items = hist_items;
    }

    gr4pm_status launch_power(const GateArgs& a, uint64_t longest)
    {
        if (longest == 0) return GR4PM_OK;
        const uint32_t groups = static_cast<uint32_t>((longest * p.B + hl::kRowGateGroupItems - 1) / hl::kRowGateGroupItems);
        hipLaunchKernelGGL(k_row_gate_power, dim3(groups, R), dim3(hl::kRowGateThreads), 0, stream, a);
        GR4PM_HIP_TRY(hipGetLastError());
        return GR4PM_OK;
    }

    // process (flush = false) or flush: validates, computes the sums, plans on copies, and commits and copies only
    // when the plan fits `cap`
    gr4pm_status run(bool flush, const gr4pm_c64* x, size_t stride, const uint64_t* lengths, gr4pm_c64* out, size_t out_stride,
                     size_t cap, gr4pm_row_gate_record* records, size_t* n_bursts)
    {
        static const uint64_t none[hl::kRowGateMaxRows] = {};
        if (flush) lengths = none, stride = 0;
        size_t at = 0;
        GR4PM_TRY(refuse(hl::row_gate_call_check(p, R, x != nullptr, stride, lengths, out != nullptr, records != nullptr,
                                                 n_bursts != nullptr, cap, &at), at));
        if (cap > 1 && out_stride < n_cols) {
            set_error("row_gate: an output stride of %zu items below the %u columns", out_stride, n_cols);
            return GR4PM_ERR_INVALID;
        }
        GR4PM_TRY(device());
        GateArgs a = {};
        base_args(a, x, stride);
        uint64_t offs[hl::kRowGateMaxRows], total = 0, longest = 0;
        uint32_t blocks[hl::kRowGateMaxRows];
        for (size_t r = 0; r < R; ++r) {
            const hl::RowGateRow& s = rows[r];
            const uint64_t lead = hl::row_gate_partial(s, p.B);
            const uint64_t nb = flush ? (lead != 0 ? 1 : 0) : hl::row_gate_blocks_for(s, p.B, lengths[r]);
            offs[r] = total, blocks[r] = static_cast<uint32_t>(nb);
            a.row[r] = GateRow{total, static_cast<uint32_t>(lengths[r]), static_cast<uint32_t>(hl::row_gate_retained(s, p.B)),
                               static_cast<uint32_t>(lead), blocks[r], s.hist, 0};
            total += nb, longest = std::max(longest, nb);
        }
        if (total != 0) {
            if (d_sums.n < total) GR4PM_TRY(d_sums.alloc(total + total / 2));
            if (h_sums.n < total) GR4PM_TRY(h_sums.alloc(total + total / 2));
            a.sums = d_sums.p;
            GR4PM_TRY(launch_power(a, longest));
            GR4PM_HIP_TRY(hipMemcpyAsync(h_sums.p, d_sums.p, total * sizeof(float), hipMemcpyDeviceToHost, stream));
        }
        GR4PM_HIP_TRY(hipStreamSynchronize(stream)); // the sums; and the span table of the call before is free again
        const size_t room = static_cast<size_t>(std::min<uint64_t>(cap, total + R)); // a span takes a block, or a row's end
        spans.resize(room), span_row.resize(room);
        const size_t count = hl::row_gate_plan_call(rows.data(), next.data(), R, p, h_sums.p, offs, blocks, lengths, flush, spans.data(),
                                                    span_row.data(), room);
        *n_bursts = count;
        if (count > cap) return refuse(hl::RowGateRefusal::capacity, 0);
        // from here on the call goes through
        if (count != 0) {
            table.resize(count);
            for (size_t i = 0; i < count; ++i) {
                const uint32_t r = span_row[i];
                const hl::RowGateRecord rec = hl::row_gate_record(spans[i], p.B, next[r].items);
                // relative to the call's first new item: at least -retained
                const int64_t k0 = -static_cast<int64_t>(rows[r].items - rec.first_item);
                table[i] = GateSpan{k0, rec.n_items, r};
                records[i] = gr4pm_row_gate_record{rec.first_item, rec.first_active_item, rec.power, r, rec.n_items, rec.active_items,
                                                   rec.flags, rec.peak, 0};
            }
            if (d_spans.n < count) GR4PM_TRY(d_spans.alloc(count + count / 2));
            GR4PM_TRY(d_spans.upload_staged(table.data(), count, stream));
            const uint32_t tiles = (n_cols + 1023u) / 1024u;
            hipLaunchKernelGGL(k_row_gate_gather, dim3(static_cast<uint32_t>(count) * tiles), dim3(hl::kRowGateThreads), 0, stream, a,
                               d_spans.p, reinterpret_cast<float2*>(out), out_stride, n_cols, tiles);
            GR4PM_HIP_TRY(hipGetLastError());
        }
        if (flush) {
            for (size_t r = 0; r < R; ++r) {
                const hl::RowGateRow done = next[r];
                hl::row_gate_start(next[r]);
                next[r].emitted = done.emitted, next[r].dropped = done.dropped, next[r].truncated = done.truncated;
                next[r].hist = done.hist;
            }
        } else {
            bool any = false;
            for (size_t r = 0; r < R; ++r) {
                a.row[r].keep_new = static_cast<uint32_t>(hl::row_gate_retained(next[r], p.B));
                any = any || a.row[r].n != 0;
            }
            if (any) {
                hipLaunchKernelGGL(k_row_gate_keep, dim3(R), dim3(hl::kRowGateThreads), 0, stream, a);
                GR4PM_HIP_TRY(hipGetLastError());
            }
        }
        rows = next;
        return GR4PM_OK;
    }
};

extern "C" {

gr4pm_status gr4pm_row_gate_create(const gr4pm_row_gate_params* q, gr4pm_row_gate** out)
try {
    if (!q || !out) return GR4PM_ERR_INVALID;
    *out = nullptr;
    hl::RowGateParams p = {};
    p.B = q->block ? q->block : 64;
    p.hold = q->hold_blocks, p.min_blocks = q->min_blocks, p.pre = q->pre_blocks, p.post = q->post_blocks;
    const uint64_t n_cols = q->n_cols;
    p.max_blocks = q->max_blocks ? q->max_blocks : static_cast<uint32_t>(std::min<uint64_t>(n_cols / p.B, UINT32_MAX));
    const hl::RowGateRefusal why = hl::row_gate_params_check(q->n_rows, p, n_cols);
    if (why != hl::RowGateRefusal::none) {
        set_error("row_gate: %zu rows, blocks of %u, hold %u, min %u, pre %u, post %u, max %u, %zu columns: %s", q->n_rows, p.B, p.hold,
                  p.min_blocks, p.pre, p.post, p.max_blocks, static_cast<size_t>(n_cols), refusal_text(why));
        return GR4PM_ERR_INVALID;
    }
    const bool unset = q->open_sum == 0.0f && q->close_sum == 0.0f; // closed until set_thresholds
    const float open_sum = unset ? INFINITY : q->open_sum, close_sum = unset ? INFINITY : q->close_sum;
    if (!hl::row_gate_thresholds_valid(open_sum, close_sum)) return refuse(hl::RowGateRefusal::thresholds, 0);
    std::unique_ptr<gr4pm_row_gate> h(new (std::nothrow) gr4pm_row_gate);
    if (!h) return GR4PM_ERR_NOMEM;
    h->p = p, h->R = static_cast<uint32_t>(q->n_rows), h->n_cols = static_cast<uint32_t>(n_cols);
    h->hist_items = static_cast<uint32_t>(hl::row_gate_retained_bound(p) + 1);
    h->stream = static_cast<hipStream_t>(q->stream);
    h->rows.resize(h->R), h->next.resize(h->R);
    for (hl::RowGateRow& s : h->rows) {
        s = hl::RowGateRow{};
        s.open_sum = open_sum, s.close_sum = close_sum;
    }
    *out = h.release();
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

void gr4pm_row_gate_destroy(gr4pm_row_gate* h)
try {
    if (!h) return;
    if (h->on_device) (void)hipStreamSynchronize(h->stream);
    delete h;
}
GR4PM_ABI_CATCH_VOID

gr4pm_status gr4pm_row_gate_reset(gr4pm_row_gate* h)
try {
    if (!h) return GR4PM_ERR_INVALID;
    h->restart();
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_row_gate_set_thresholds(gr4pm_row_gate* h, size_t row, float open_sum, float close_sum)
try {
    if (!h) return GR4PM_ERR_INVALID;
    if (row >= h->R) {
        set_error("row_gate: row %zu of %u", row, h->R);
        return GR4PM_ERR_INVALID;
    }
    if (!hl::row_gate_thresholds_valid(open_sum, close_sum)) return refuse(hl::RowGateRefusal::thresholds, row);
    h->rows[row].open_sum = open_sum, h->rows[row].close_sum = close_sum;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_row_gate_state(const gr4pm_row_gate* h, size_t row, gr4pm_row_gate_state_t* out)
try {
    if (!h || row >= h->R || !out) return GR4PM_ERR_INVALID;
    const hl::RowGateRow& s = h->rows[row];
    *out = gr4pm_row_gate_state_t{s.items, s.decided, s.emitted, s.dropped, s.truncated, s.open, 0};
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_row_gate_sizes(const gr4pm_row_gate* h, uint32_t* block, uint32_t* max_blocks, size_t* n_cols)
try {
    if (!h || !block || !max_blocks || !n_cols) return GR4PM_ERR_INVALID;
    *block = h->p.B, *max_blocks = h->p.max_blocks, *n_cols = h->n_cols;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_row_gate_process(gr4pm_row_gate* h, const gr4pm_c64* x, size_t stride, const uint64_t* lengths, gr4pm_c64* out,
                                    size_t out_stride, size_t cap, gr4pm_row_gate_record* records, size_t* n_bursts)
try {
    if (!h) return GR4PM_ERR_INVALID;
    return h->run(false, x, stride, lengths, out, out_stride, cap, records, n_bursts);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_row_gate_flush(gr4pm_row_gate* h, gr4pm_c64* out, size_t out_stride, size_t cap, gr4pm_row_gate_record* records,
                                  size_t* n_bursts)
try {
    if (!h) return GR4PM_ERR_INVALID;
    return h->run(true, nullptr, 0, nullptr, out, out_stride, cap, records, n_bursts);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_row_gate_block_power(gr4pm_row_gate* h, const gr4pm_c64* x, size_t stride, const uint64_t* lengths, float* out,
                                        size_t out_stride)
try {
    if (!h) return GR4PM_ERR_INVALID;
    if (!lengths || !out) return refuse(hl::RowGateRefusal::pointer, 0);
    uint64_t longest = 0;
    bool any = false;
    for (size_t r = 0; r < h->R; ++r) {
        if (lengths[r] > stride) return refuse(hl::RowGateRefusal::length, r);
        if (!hl::row_gate_length_valid(lengths[r], h->p)) return refuse(hl::RowGateRefusal::items, r);
        if (h->R > 1 && lengths[r] / h->p.B > out_stride) return refuse(hl::RowGateRefusal::length, r);
        longest = std::max(longest, lengths[r] / h->p.B);
        any = any || lengths[r] != 0;
    }
    if (any && !x) return refuse(hl::RowGateRefusal::pointer, 0);
    GR4PM_TRY(h->device());
    GateArgs a = {};
    h->base_args(a, x, stride);
    a.sums = out;
    for (size_t r = 0; r < h->R; ++r)
        a.row[r] = GateRow{r * static_cast<uint64_t>(out_stride), static_cast<uint32_t>(lengths[r]), 0, 0,
                           static_cast<uint32_t>(lengths[r] / h->p.B), 0, 0};
    return h->launch_power(a, longest);
}
GR4PM_ABI_CATCH

} // extern "C"
