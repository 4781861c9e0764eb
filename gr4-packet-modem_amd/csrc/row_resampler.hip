// row_resampler.hip -- rows of channel items to any real rate with the residual carrier removed, every row with a step
// and a frequency of its own: what acts on a LineSpectrum's per-row symbol rate and offset where they were measured, on
// the burst rows of gr4pm_ddc_extract.  The project's own block (the reference's PfbArbResampler is one stream per handle,
// a float accumulator recurrence serial in the stream position, and no mixer).  Definition: include/gr4pm_hip.h,
// DESIGN.md section 24; positions, lengths, the tile and the call's validation: hostlogic/row_resample_plan.hpp.
//
// k_row_resample is row_kernel.hpp's body on rows that are not carried: a call is a stream call on fresh rows (d = phase0,
// no history), and its argument block hands the body's per-row record over that way, from the gr4pm_row_record, n_r and
// M_r it holds.  The kernel, the design and the handle's table are described there.
#include "row_kernel.hpp"

namespace {

using namespace gr4pm;
namespace hl = gr4pm::hostlogic;

struct OneShotArgs { // fresh rows: the records as the call brings them, d = phase0 and no history
    static constexpr bool carried = false;
    const float2* x;
    float2* out;
    const float2* tab; // [P][Q] of {H[q][s], Dh[q][s]}
    size_t stride, out_stride;
    uint32_t n_cols_out;
    uint32_t Q, P, b, T;
    uint32_t n[hl::kRowMaxRows];
    uint32_t M[hl::kRowMaxRows];
    hl::RowRecord rec[hl::kRowMaxRows];
    __device__ uint32_t items_out(uint32_t r) const { return M[r]; }
    __device__ RowItem item(uint32_t r) const { return RowItem{rec[r].phase0, rec[r].step, rec[r].freq, 0, 0, n[r], M[r], 0}; }
};
static_assert(sizeof(OneShotArgs) <= 4096, "the argument block");

__global__ __launch_bounds__(hl::kRowThreads) void k_row_resample(OneShotArgs a)
{
    extern __shared__ float2 s_row[];
    row_body(a, s_row);
}

} // namespace

struct gr4pm_row_resampler {
    uint32_t Q = 0, P = 0;
    hipStream_t stream = nullptr;
    gr4pm::DevBuf<float2> d_tab;
};

extern "C" {

gr4pm_status gr4pm_row_resampler_taps(size_t phases, size_t taps_per_phase, double max_step, double passband, double stopband,
                                      float* out)
try {
    if (!out) return GR4PM_ERR_INVALID;
    std::vector<double> h;
    GR4PM_TRY(row_design(phases, taps_per_phase, max_step, passband, stopband, h));
    for (size_t t = 0; t < h.size(); ++t) out[t] = static_cast<float>(h[t]);
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_row_resampler_create(const gr4pm_row_resampler_params* p, gr4pm_row_resampler** out)
try {
    if (!p || !out) return GR4PM_ERR_INVALID;
    *out = nullptr;
    uint32_t Q, P;
    std::vector<float2> tab;
    GR4PM_TRY(row_table("row_resampler", p->phases, p->taps_per_phase, p->taps, Q, P, tab));
    GR4PM_TRY(require_device());
    std::unique_ptr<gr4pm_row_resampler> h(new (std::nothrow) gr4pm_row_resampler);
    if (!h) return GR4PM_ERR_NOMEM;
    h->Q = Q, h->P = P;
    h->stream = static_cast<hipStream_t>(p->stream);
    GR4PM_TRY(h->d_tab.alloc(tab.size()));
    GR4PM_TRY(h->d_tab.upload(tab.data(), tab.size(), h->stream));
    GR4PM_TRY(raise_dynamic_lds({reinterpret_cast<const void*>(&k_row_resample)},
                                (hl::kRowMaxTaps + hl::kRowStageItems) * sizeof(float2), "row_resampler"));
    return finish_create(h, out, "row_resampler");
}
GR4PM_ABI_CATCH

void gr4pm_row_resampler_destroy(gr4pm_row_resampler* h)
try {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    delete h;
}
GR4PM_ABI_CATCH_VOID

gr4pm_status gr4pm_row_resampler_output_lengths(size_t taps_per_phase, size_t n_cols, const uint64_t* lengths,
                                                const gr4pm_row_record* rows, size_t n_rows, size_t n_cols_out,
                                                uint64_t* out_lengths)
try {
    if (taps_per_phase < 1 || taps_per_phase > hl::kRowMaxTaps / hl::kRowMinPhases) {
        set_error("row_resampler: %zu taps per phase", taps_per_phase);
        return GR4PM_ERR_INVALID;
    }
    // what the call would decide, with arrays that are not looked at counted as present and one row's strides
    const hl::RowPlan p = hl::row_plan(taps_per_phase, true, n_cols, n_cols, lengths, rows, n_rows, true, n_cols_out, n_cols_out,
                                       out_lengths != nullptr);
    GR4PM_TRY(row_refusal_status(p.why, p.at, false));
    for (size_t r = 0; r < n_rows; ++r) out_lengths[r] = p.M[r];
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

uint32_t gr4pm_row_resampler_tile_items(size_t taps_per_phase, uint64_t max_step)
try {
    if (taps_per_phase < 1 || taps_per_phase > hl::kRowMaxTaps / hl::kRowMinPhases || !hl::row_step_valid(max_step)) return 0;
    return hl::row_tile(taps_per_phase, max_step);
}
GR4PM_ABI_CATCH_RET(0)

gr4pm_status gr4pm_row_resampler_process(gr4pm_row_resampler* h, const gr4pm_c64* x, size_t stride, size_t n_cols,
                                         const uint64_t* lengths, const gr4pm_row_record* rows, size_t n_rows, gr4pm_c64* out,
                                         size_t out_stride, size_t n_cols_out, uint64_t* out_lengths)
try {
    if (!h) return GR4PM_ERR_INVALID;
    const hl::RowPlan p = hl::row_plan(h->P, x != nullptr, stride, n_cols, lengths, rows, n_rows, out != nullptr, out_stride,
                                       n_cols_out, out_lengths != nullptr);
    GR4PM_TRY(row_refusal_status(p.why, p.at, false));
    if (p.why == hl::RowRefusal::nothing) {
        if (out_lengths && rows && n_rows <= hl::kRowMaxRows)
            for (size_t r = 0; r < n_rows; ++r) out_lengths[r] = 0; // no column
        return GR4PM_OK;
    }
    OneShotArgs a = {};
    a.x = reinterpret_cast<const float2*>(x), a.out = reinterpret_cast<float2*>(out), a.tab = h->d_tab.p;
    a.stride = stride, a.out_stride = out_stride;
    a.n_cols_out = static_cast<uint32_t>(n_cols_out);
    a.Q = h->Q, a.P = h->P, a.b = 32 - hl::row_log2(h->Q), a.T = p.T;
    uint64_t max_step = 0;
    for (size_t r = 0; r < n_rows; ++r) {
        a.n[r] = p.n[r], a.M[r] = p.M[r], a.rec[r] = rows[r]; // M from row_plan: 0 for a row of no items, and cut at n_cols_out
        out_lengths[r] = p.M[r];
        max_step = std::max(max_step, rows[r].step);
    }
    // the tables and the span a tile of T items can have at the call's largest step (row_tile() keeps it within the stage)
    const size_t smem = (static_cast<size_t>(h->Q) * h->P + hl::row_span_bound(p.T, max_step, h->P)) * sizeof(float2);
    hipLaunchKernelGGL(k_row_resample, dim3(p.grid_x, p.grid_y), dim3(hl::kRowThreads), smem, h->stream, a);
    GR4PM_HIP_TRY(hipGetLastError());
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

} // extern "C"
