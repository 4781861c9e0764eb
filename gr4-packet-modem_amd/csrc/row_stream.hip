// row_stream.hip -- the RowResampler as a stream block: every row's position, history and phase are carried from call to
// call, so that cutting the rows into calls changes no bit of what comes out (the one-shot block of row_resampler.hip,
// which stays as it is, is the yardstick).  Definition: include/gr4pm_hip.h; the carried state,
// the counts, the rebase, set_row and the call's validation: hostlogic/row_stream_plan.hpp, whose expressions the kernels
// use.
//
// k_row_stream: the grid of k_row_resample: blockIdx.y is the row, blockIdx.x a tile of T output items of this call.  A
//   row's state travels by value: d (the position of the call's first item relative to the row's next input item), the
//   step, the frequency word, Phi, the fraction of the phase reference, the call's items and count.  The workgroup copies
//   the table and the tile's span to LDS; the span comes from two places: stage items in front of the call's first input
//   item read the row's history buffer (its last P - 1 items), the rest read x_r, and an index at or behind lengths[r] is
//   staged as +0 by an explicit range test and not loaded (only flush reaches those).  The tap loop, the LDS layout
//   [s][q] of {H, Dh} and the rotator are k_row_resample's, expression by expression; the rotator's operand is Phi +
//   row_theta(freq, pos - ref).  No pass copies the new items beside the history first.
// k_row_stream_keep: one workgroup per row writes the row's new last P - 1 items, from the old history and x_r, into the
//   other of the row's two history buffers (with lengths[r] < P - 1 source and destination would overlap).  A row with
//   lengths[r] = 0 keeps its buffer.
// Built with EXACT_FLAGS: every fmaf is written out, nothing else contracts.
#include "freq_xlate.hpp"
#include "hostlogic/row_stream_plan.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

using namespace gr4pm;
namespace hl = gr4pm::hostlogic;

struct StreamRow { // 40 bytes: 64 of them and the header stay well inside the 4 KiB of kernel arguments
    uint64_t d, step;
    int32_t freq;
    uint32_t phi, ref_frac;
    uint32_t n, M; // the call's input and output items
    uint32_t hist; // the buffer that holds the history the call reads
};

struct StreamArgs {
    const float2* x;
    float2* out;
    const float2* tab; // [P][Q] of {H[q][s], Dh[q][s]}
    float2* hist;      // [2][R][P - 1]
    size_t stride, out_stride;
    uint32_t n_cols_out;
    uint32_t Q, P, b, T, R;
    StreamRow row[hl::kRowMaxRows];
};
static_assert(sizeof(StreamArgs) <= 4096, "the argument block");

__device__ __forceinline__ float2* history_of(const StreamArgs& a, uint32_t buf, uint32_t r)
{
    return a.hist + (static_cast<size_t>(buf) * a.R + r) * (a.P - 1);
}

__global__ __launch_bounds__(hl::kRowThreads) void k_row_stream(StreamArgs a)
{
    extern __shared__ float2 s_row[];
    const uint32_t tid = threadIdx.x;
    const uint32_t Q = a.Q, P = a.P, T = a.T, r = blockIdx.y;
    const uint32_t m0 = blockIdx.x * T; // below n_cols_out <= 2^31
    const uint32_t nv = hl::row_tile_items(m0, a.row[r].M, T);
    float2* __restrict__ row = a.out + static_cast<size_t>(r) * a.out_stride;
    if (nv == 0) { // wholly at or behind the call's count
        for (uint32_t m = tid; m < T && m0 + m < a.n_cols_out; m += hl::kRowThreads) row[m0 + m] = float2{0.0f, 0.0f};
        return;
    }
    const StreamRow rec = a.row[r];
    const uint64_t n = rec.n;
    float2* tab = s_row;
    float2* st = s_row + Q * P;
    for (uint32_t i = tid; i < Q * P; i += hl::kRowThreads) tab[i] = a.tab[i];
    // positions are relative to the row's next input item; stage item j is the item i0 - (P - 1) + j from there
    const uint64_t pos0 = rec.d + static_cast<uint64_t>(m0) * rec.step;
    const uint64_t i0 = pos0 >> 32;
    const int64_t base = static_cast<int64_t>(i0) - static_cast<int64_t>(P - 1);
    const uint32_t S = static_cast<uint32_t>(hl::row_tile_span(pos0, nv, rec.step, P));
    const float2* __restrict__ xr = a.x + static_cast<size_t>(r) * a.stride;
    const float2* __restrict__ hr = history_of(a, rec.hist, r);
    for (uint32_t j = tid; j < S; j += hl::kRowThreads) {
        const int64_t k = base + j;
        float2 v = {0.0f, 0.0f};
        switch (hl::row_stream_source(k, n)) {
        case hl::RowStreamSource::history: v = hr[static_cast<int64_t>(P - 1) + k]; break;
        case hl::RowStreamSource::input: v = xr[k]; break;
        default: break;
        }
        st[j] = v;
    }
    __syncthreads();
    const float scale = 1.0f / static_cast<float>(uint64_t(1) << a.b); // 2^-b, exact
    for (uint32_t m = tid; m < T && m0 + m < a.n_cols_out; m += hl::kRowThreads) {
        float2 y = {0.0f, 0.0f};
        if (m < nv) {
            const uint64_t pos = pos0 + static_cast<uint64_t>(m) * rec.step;
            const uint32_t mu = static_cast<uint32_t>(pos);
            const float alpha = static_cast<float>(hl::row_alpha_bits(mu, a.b)) * scale;
            const float2* tp = tab + hl::row_branch(mu, a.b);
            const float2* sp = st + (static_cast<uint32_t>((pos >> 32) - i0) + (P - 1));
            float2 acc = {0.0f, 0.0f};
#pragma unroll 4
            for (uint32_t s = 0; s < P; ++s, tp += Q, --sp) {
                const float2 hd = *tp, x = *sp;
                const float c = fmaf(alpha, hd.y, hd.x);
                acc.x = fmaf(c, x.x, acc.x);
                acc.y = fmaf(c, x.y, acc.y);
            }
            const uint32_t theta = rec.phi + hl::row_theta(rec.freq, hl::row_stream_theta_pos(pos, rec.ref_frac));
            cmac(y, mixer<-1>(theta, 1u), acc);
        }
        row[m0 + m] = y;
    }
}

__global__ __launch_bounds__(hl::kRowThreads) void k_row_stream_keep(StreamArgs a)
{
    const uint32_t r = blockIdx.x, P = a.P;
    const uint64_t n = a.row[r].n;
    if (n == 0) return; // the row keeps its buffer
    const uint32_t from = a.row[r].hist;
    const float2* __restrict__ old = history_of(a, from, r);
    float2* __restrict__ now = history_of(a, from ^ 1u, r);
    const float2* __restrict__ xr = a.x + static_cast<size_t>(r) * a.stride;
    for (uint32_t j = threadIdx.x; j < P - 1; j += hl::kRowThreads) {
        const int64_t k = hl::row_stream_keep_index(n, P, j); // in [-(P - 1), n)
        now[j] = k < 0 ? old[static_cast<int64_t>(P - 1) + k] : xr[k];
    }
}

const char* refusal_text(hl::RowStreamRefusal why)
{
    switch (why) {
    case hl::RowStreamRefusal::length: return "the row's length exceeds the columns of the input";
    case hl::RowStreamRefusal::items: return "the row's length plus the taps per phase reaches 2^32";
    case hl::RowStreamRefusal::columns: return "more than 2^31 output columns";
    case hl::RowStreamRefusal::stride: return "a row stride below the column count";
    case hl::RowStreamRefusal::lengths: return "no out_lengths array";
    case hl::RowStreamRefusal::room: return "the row makes more items in this call than the output has columns; a stream loses none";
    case hl::RowStreamRefusal::output: return "no output array";
    case hl::RowStreamRefusal::input: return "no input array";
    default: return "";
    }
}

gr4pm_status refusal_status(const hl::RowStreamPlan& p)
{
    switch (p.why) {
    case hl::RowStreamRefusal::none: return GR4PM_OK;
    case hl::RowStreamRefusal::items:
    case hl::RowStreamRefusal::columns:
    case hl::RowStreamRefusal::room:
        set_error("row_stream: row %zu: %s", p.at, refusal_text(p.why));
        return GR4PM_ERR_OVERFLOW;
    default: set_error("row_stream: row %zu: %s", p.at, refusal_text(p.why)); return GR4PM_ERR_INVALID;
    }
}

} // namespace

struct gr4pm_row_stream {
    uint32_t Q = 0, P = 0, R = 0;
    hipStream_t stream = nullptr;
    bool on_device = false; // the tables and the histories are made by the first call that enqueues: create, items_for,
                            // set_row, state and reset of a handle that has not run yet are host only
    std::vector<float2> tab;
    gr4pm::DevBuf<float2> d_tab, d_hist;
    std::vector<hl::RowStreamRow> rows;

    gr4pm_status device()
    {
        if (on_device) return GR4PM_OK;
        GR4PM_TRY(require_device());
        GR4PM_TRY(d_tab.alloc(tab.size()));
        GR4PM_TRY(d_tab.upload(tab.data(), tab.size(), stream));
        GR4PM_TRY(d_hist.alloc(2 * static_cast<size_t>(R) * (P - 1)));
        GR4PM_TRY(d_hist.zero(stream));
        GR4PM_TRY(raise_dynamic_lds({reinterpret_cast<const void*>(&k_row_stream)},
                                    (hl::kRowMaxTaps + hl::kRowStageItems) * sizeof(float2), "row_stream"));
        GR4PM_HIP_TRY(hipStreamSynchronize(stream)); // the upload reads `tab`
        on_device = true;
        return GR4PM_OK;
    }

    gr4pm_status restart() // every row back to its created state, with its current step and freq
    {
        if (on_device) GR4PM_TRY(d_hist.zero(stream));
        for (hl::RowStreamRow& s : rows) {
            s.hist = 0;
            hl::row_stream_start(s);
        }
        return GR4PM_OK;
    }

    // process (flush = false) or the output of a flush: validates, launches and, behind a launch that went out, advances
    gr4pm_status run(bool flush, const gr4pm_c64* x, size_t stride, size_t n_cols, const uint64_t* lengths, gr4pm_c64* out,
                     size_t out_stride, size_t n_cols_out, uint64_t* out_lengths)
    {
        const hl::RowStreamPlan p = hl::row_stream_plan(rows.data(), R, P, flush, x != nullptr, stride, n_cols, lengths,
                                                        out != nullptr, out_stride, n_cols_out, out_lengths != nullptr);
        GR4PM_TRY(refusal_status(p));
        GR4PM_TRY(device());
        StreamArgs a = {};
        a.x = reinterpret_cast<const float2*>(x), a.out = reinterpret_cast<float2*>(out), a.tab = d_tab.p, a.hist = d_hist.p;
        a.stride = stride, a.out_stride = out_stride;
        a.n_cols_out = static_cast<uint32_t>(n_cols_out);
        a.Q = Q, a.P = P, a.b = 32 - hl::row_log2(Q), a.T = p.T, a.R = R;
        uint64_t max_step = 0;
        bool any = false;
        for (size_t r = 0; r < R; ++r) {
            const hl::RowStreamRow& s = rows[r];
            a.row[r] = StreamRow{s.d, s.step, s.freq, s.phi, s.ref_frac, p.n[r], p.M[r], s.hist};
            max_step = std::max(max_step, s.step);
            any = any || p.n[r] != 0;
        }
        if (p.grid_x != 0) {
            const size_t smem = (static_cast<size_t>(Q) * P + hl::row_span_bound(p.T, max_step, P)) * sizeof(float2);
            hipLaunchKernelGGL(k_row_stream, dim3(p.grid_x, p.grid_y), dim3(hl::kRowThreads), smem, stream, a);
            GR4PM_HIP_TRY(hipGetLastError());
        }
        if (any && P > 1) {
            hipLaunchKernelGGL(k_row_stream_keep, dim3(R), dim3(hl::kRowThreads), 0, stream, a);
            GR4PM_HIP_TRY(hipGetLastError());
        }
        for (size_t r = 0; r < R; ++r) {
            out_lengths[r] = p.M[r];
            if (!flush) hl::row_stream_advance(rows[r], p.n[r], p.M[r]);
        }
        return flush ? restart() : GR4PM_OK;
    }
};

extern "C" {

gr4pm_status gr4pm_row_stream_create(const gr4pm_row_stream_params* p, gr4pm_row_stream** out)
try {
    if (!p || !out) return GR4PM_ERR_INVALID;
    *out = nullptr;
    const size_t Q = p->phases, P = p->taps_per_phase ? p->taps_per_phase : (p->taps ? 0 : 12), R = p->n_rows;
    if (!hl::row_sizes_valid(Q, P)) {
        set_error("row_stream: %zu phases of %zu taps: the phases are a power of two in [%u, %u], and there are 1 .. %zu taps in all",
                  Q, P, hl::kRowMinPhases, hl::kRowMaxPhases, hl::kRowMaxTaps);
        return GR4PM_ERR_INVALID;
    }
    if (R < 1 || R > hl::kRowMaxRows || !p->rows) {
        set_error("row_stream: %zu rows%s: a handle has 1 .. %zu rows and a record for each", R, p->rows ? "" : " and no records",
                  hl::kRowMaxRows);
        return GR4PM_ERR_INVALID;
    }
    for (size_t r = 0; r < R; ++r) {
        if (!hl::row_step_valid(p->rows[r].step)) {
            set_error("row_stream: row %zu: the step is outside 2^26 .. 2^38 (1/64 .. 64 input items per output item)", r);
            return GR4PM_ERR_INVALID;
        }
        if (p->rows[r].phase0 >= (uint64_t(1) << 63)) {
            set_error("row_stream: row %zu: phase0 is 2^63 or more", r);
            return GR4PM_ERR_OVERFLOW;
        }
    }
    std::vector<float> taps(Q * P + 1, 0.0f); // h[Q P] = 0
    if (p->taps)
        std::copy(p->taps, p->taps + Q * P, taps.begin());
    else
        GR4PM_TRY(gr4pm_row_resampler_taps(Q, P, 1.0, 0.25, 0.75, taps.data())); // the one-shot block's default design
    for (size_t t = 0; t < Q * P; ++t)
        if (!std::isfinite(taps[t])) {
            set_error("row_stream: taps[%zu] is not finite", t);
            return GR4PM_ERR_INVALID;
        }
    std::unique_ptr<gr4pm_row_stream> h(new (std::nothrow) gr4pm_row_stream);
    if (!h) return GR4PM_ERR_NOMEM;
    h->Q = static_cast<uint32_t>(Q), h->P = static_cast<uint32_t>(P), h->R = static_cast<uint32_t>(R);
    h->stream = static_cast<hipStream_t>(p->stream);
    h->tab.resize(Q * P);
    for (size_t s = 0; s < P; ++s)
        for (size_t q = 0; q < Q; ++q) {
            const size_t t = s * Q + q;
            const double d = static_cast<double>(taps[t + 1]) - static_cast<double>(taps[t]);
            h->tab[t] = float2{taps[t], static_cast<float>(d)};
        }
    h->rows.resize(R);
    for (size_t r = 0; r < R; ++r) {
        hl::RowStreamRow& s = h->rows[r];
        s = hl::RowStreamRow{};
        s.step = p->rows[r].step, s.phase0 = p->rows[r].phase0, s.freq = p->rows[r].freq;
        s.start = p->start_index ? p->start_index[r] : 0;
    }
    GR4PM_TRY(h->restart());
    *out = h.release();
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

void gr4pm_row_stream_destroy(gr4pm_row_stream* h)
try {
    if (!h) return;
    if (h->on_device) (void)hipStreamSynchronize(h->stream);
    delete h;
}
GR4PM_ABI_CATCH_VOID

gr4pm_status gr4pm_row_stream_reset(gr4pm_row_stream* h)
try {
    if (!h) return GR4PM_ERR_INVALID;
    return h->restart();
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_row_stream_items_for(const gr4pm_row_stream* h, const uint64_t* lengths, uint64_t* out_lengths)
try {
    if (!h || !lengths || !out_lengths) return GR4PM_ERR_INVALID;
    for (size_t r = 0; r < h->R; ++r)
        if (!hl::row_stream_items_valid(lengths[r], h->P)) {
            set_error("row_stream: row %zu: %s", r, refusal_text(hl::RowStreamRefusal::items));
            return GR4PM_ERR_OVERFLOW;
        }
    for (size_t r = 0; r < h->R; ++r) out_lengths[r] = hl::row_stream_count(h->rows[r], lengths[r]);
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_row_stream_process(gr4pm_row_stream* h, const gr4pm_c64* x, size_t stride, size_t n_cols, const uint64_t* lengths,
                                      gr4pm_c64* out, size_t out_stride, size_t n_cols_out, uint64_t* out_lengths)
try {
    if (!h) return GR4PM_ERR_INVALID;
    return h->run(false, x, stride, n_cols, lengths, out, out_stride, n_cols_out, out_lengths);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_row_stream_flush(gr4pm_row_stream* h, gr4pm_c64* out, size_t out_stride, size_t n_cols_out, uint64_t* out_lengths)
try {
    if (!h) return GR4PM_ERR_INVALID;
    return h->run(true, nullptr, 0, 0, nullptr, out, out_stride, n_cols_out, out_lengths);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_row_stream_set_row(gr4pm_row_stream* h, size_t row, uint64_t step, int32_t freq)
try {
    if (!h) return GR4PM_ERR_INVALID;
    if (row >= h->R) {
        set_error("row_stream: row %zu of %u", row, h->R);
        return GR4PM_ERR_INVALID;
    }
    if (!hl::row_step_valid(step)) {
        set_error("row_stream: row %zu: the step is outside 2^26 .. 2^38 (1/64 .. 64 input items per output item)", row);
        return GR4PM_ERR_INVALID;
    }
    hl::row_stream_retune(h->rows[row], step, freq);
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_row_stream_state(const gr4pm_row_stream* h, size_t row, uint64_t* items_in, uint64_t* items_out)
try {
    if (!h || row >= h->R || !items_in || !items_out) return GR4PM_ERR_INVALID;
    *items_in = h->rows[row].items_in, *items_out = h->rows[row].items_out;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

} // extern "C"
