// row_stream.hip -- the RowResampler as a stream block: every row's position, history and phase are carried from call to
// call, so that cutting the rows into calls changes no bit of what comes out.  Definition: include/gr4pm_hip.h, DESIGN.md
// section 29; the carried state, the counts, the rebase, set_row and the call's validation:
// hostlogic/row_stream_plan.hpp, whose expressions the kernels use.
//
// k_row_stream is row_kernel.hpp's body on carried rows.  A row's state travels by value: d (the position of the call's
//   first item relative to the row's next input item), the step, the frequency word, Phi, the fraction of the phase
//   reference, the call's items and count; stage items in front of the call's first input item read the row's history
//   buffer, and the rotator's operand is Phi + row_theta(freq, pos - ref).  No pass copies the new items beside the
//   history first.  The one-shot block's k_row_resample (row_resampler.hip) is the same body on fresh rows.
// k_row_stream_keep: one workgroup per row writes the row's new last P - 1 items, from the old history and x_r, into the
//   other of the row's two history buffers (with lengths[r] < P - 1 source and destination would overlap).  A row with
//   lengths[r] = 0 keeps its buffer.
// Built with EXACT_FLAGS: every fmaf is written out, nothing else contracts.
#include "row_kernel.hpp"

namespace {

using namespace gr4pm;
namespace hl = gr4pm::hostlogic;

__global__ __launch_bounds__(hl::kRowThreads) void k_row_stream(RowArgs a)
{
    extern __shared__ float2 s_row[];
    row_body(a, s_row);
}

__global__ __launch_bounds__(hl::kRowThreads) void k_row_stream_keep(RowArgs a)
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
        GR4PM_TRY(row_refusal_status(p.why, p.at, true));
        GR4PM_TRY(device());
        RowArgs a = {};
        a.x = reinterpret_cast<const float2*>(x), a.out = reinterpret_cast<float2*>(out), a.tab = d_tab.p, a.hist = d_hist.p;
        a.stride = stride, a.out_stride = out_stride;
        a.n_cols_out = static_cast<uint32_t>(n_cols_out);
        a.Q = Q, a.P = P, a.b = 32 - hl::row_log2(Q), a.T = p.T, a.R = R;
        uint64_t max_step = 0;
        bool any = false;
        for (size_t r = 0; r < R; ++r) {
            const hl::RowStreamRow& s = rows[r];
            a.row[r] = RowItem{s.d, s.step, s.freq, s.phi, s.ref_frac, p.n[r], p.M[r], s.hist};
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
    uint32_t Q, P;
    std::vector<float2> tab;
    GR4PM_TRY(row_table("row_stream", p->phases, p->taps_per_phase, p->taps, Q, P, tab));
    const size_t R = p->n_rows;
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
    std::unique_ptr<gr4pm_row_stream> h(new (std::nothrow) gr4pm_row_stream);
    if (!h) return GR4PM_ERR_NOMEM;
    h->Q = Q, h->P = P, h->R = static_cast<uint32_t>(R);
    h->stream = static_cast<hipStream_t>(p->stream);
    h->tab = std::move(tab);
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
            set_error("row_stream: row %zu: %s", r, row_refusal_text(hl::RowRefusal::items, true));
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
