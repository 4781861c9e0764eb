// row_resampler.hip -- rows of channel items to any real rate with the residual carrier removed, every row with a step
// and a frequency of its own: what acts on a LineSpectrum's per-row symbol rate and offset where they were measured, on
// the burst rows of gr4pm_ddc_extract.  The project's own block (the reference's PfbArbResampler is one stream per handle,
// a float accumulator recurrence serial in the stream position, and no mixer).  Definition: include/gr4pm_hip.h,
// DESIGN.md section 24; positions, lengths, the tile and the call's validation: hostlogic/row_resample_plan.hpp, whose
// expressions the kernel uses.
//
// k_row_resample: blockIdx.y is the row, blockIdx.x a tile of T output items (T <= 1024, picked by the host from the
//   call's largest step so that the tile's input span fits the stage).  The row's record, its lengths and the tile's first
//   position are wave-uniform.  The workgroup copies the handle's coefficient table and the tile's input span to LDS once;
//   an index outside [0, n_r) is staged as +0 by an explicit range test and never loaded.  Lanes then take consecutive
//   output items, four per thread at the full tile.  Each lane has its own branch q and fraction alpha, so the
//   coefficients are per-lane LDS reads: one 8-byte read of {H, Dh}[s][q] and one of the sample per tap, three fmaf.
//   The table is laid out [s][q], q fastest, the pair {H, Dh} in one float2: the ds_read_b64 of a tap takes the bank pair
//   q mod 32 in a half-wave of 32 lanes, so for Q <= 32 any pattern of q is conflict-free (equal q is one address and
//   broadcasts); Q = 64 .. 256 can put q and q + 32 k on one bank pair.  [q][s] with P = 12 would leave 12 q mod 32 only
//   eight bank pairs.  A tile wholly at or behind M_r stores zeros and stages nothing.
// Nothing depends on the tile an item falls in or on the rows beside it: every item is a function of (row, pos) alone.
// Built with EXACT_FLAGS: every fmaf is written out, nothing else contracts.
#include "freq_xlate.hpp"
#include "hostlogic/row_resample_plan.hpp"
#include "kaiser_design.hpp"

#include <algorithm>
#include <cmath>

namespace {

using namespace gr4pm;
namespace hl = gr4pm::hostlogic;

struct RowArgs {
    const float2* x;
    float2* out;
    const float2* tab;   // [P][Q] of {H[q][s], Dh[q][s]}
    size_t stride, out_stride;
    uint32_t n_cols_out;
    uint32_t Q, P, b, T;
    uint32_t n[hl::kRowMaxRows];
    uint32_t M[hl::kRowMaxRows];
    hl::RowRecord rec[hl::kRowMaxRows];
};

__global__ __launch_bounds__(hl::kRowThreads) void k_row_resample(RowArgs a)
{
    extern __shared__ float2 s_row[];
    const uint32_t tid = threadIdx.x;
    const uint32_t Q = a.Q, P = a.P, T = a.T, r = blockIdx.y;
    const uint32_t m0 = blockIdx.x * T; // below n_cols_out <= 2^31
    const uint32_t nv = hl::row_tile_items(m0, a.M[r], T);
    float2* __restrict__ row = a.out + static_cast<size_t>(r) * a.out_stride;
    if (nv == 0) { // wholly at or behind the row's end
        for (uint32_t m = tid; m < T && m0 + m < a.n_cols_out; m += hl::kRowThreads) row[m0 + m] = float2{0.0f, 0.0f};
        return;
    }
    const hl::RowRecord rec = a.rec[r];
    const uint64_t n = a.n[r];
    float2* tab = s_row;
    float2* st = s_row + Q * P;
    for (uint32_t i = tid; i < Q * P; i += hl::kRowThreads) tab[i] = a.tab[i];
    // stage item j: input index base + j of the row; the tile's first item takes its oldest sample from j = 0
    const uint64_t pos0 = rec.phase0 + static_cast<uint64_t>(m0) * rec.step;
    const uint64_t i0 = pos0 >> 32;
    const int64_t base = static_cast<int64_t>(i0) - static_cast<int64_t>(P - 1);
    const uint32_t S = static_cast<uint32_t>(hl::row_tile_span(pos0, nv, rec.step, P));
    const float2* __restrict__ xr = a.x + static_cast<size_t>(r) * a.stride;
    for (uint32_t j = tid; j < S; j += hl::kRowThreads) {
        const int64_t k = base + j;
        float2 v = {0.0f, 0.0f};
        if (hl::row_item_loaded(k, n)) v = xr[k];
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
            cmac(y, mixer<-1>(hl::row_theta(rec.freq, pos), 1u), acc);
        }
        row[m0 + m] = y;
    }
}

bool sizes_or_error(const char* what, size_t Q, size_t P)
{
    if (hl::row_sizes_valid(Q, P)) return true;
    set_error("%s: %zu phases of %zu taps: the phases are a power of two in [%u, %u], and there are 1 .. %zu taps in all", what, Q,
              P, hl::kRowMinPhases, hl::kRowMaxPhases, hl::kRowMaxTaps);
    return false;
}

gr4pm_status design(size_t Q, size_t per, double max_step, double passband, double stopband, std::vector<double>& h)
{
    if (!(max_step >= 1.0 / 64.0 && max_step <= 64.0)) { // a NaN fails
        set_error("row_resampler: max_step is %g, need 1/64 .. 64 input items per output item", max_step);
        return GR4PM_ERR_INVALID;
    }
    if (per < 1 || per > hl::kRowMaxTaps) {
        set_error("row_resampler: %zu taps per phase, need 1 .. %zu / phases", per, hl::kRowMaxTaps);
        return GR4PM_ERR_INVALID;
    }
    const double widen = std::max(1.0, max_step);
    const double span = std::ceil(static_cast<double>(per) * widen); // at most 4096 * 64
    if (!sizes_or_error("row_resampler", Q, static_cast<size_t>(span))) return GR4PM_ERR_INVALID;
    if (!(passband >= 0.0 && passband < stopband && passband + stopband <= 1.0)) {
        set_error("row_resampler: need 0 <= passband < stopband (units of the lower of the input and the output rate) and a "
                  "cutoff of at most half of it: passband + stopband <= 1");
        return GR4PM_ERR_INVALID;
    }
    const size_t P = static_cast<size_t>(span);
    kaiser_lowpass(Q * P, Q, passband / widen, stopband / widen, h, static_cast<double>(Q));
    return GR4PM_OK;
}

const char* refusal_text(hl::RowRefusal why)
{
    switch (why) {
    case hl::RowRefusal::rows: return "at most 64 rows go into one call";
    case hl::RowRefusal::records: return "no array of row records";
    case hl::RowRefusal::length: return "a row's length exceeds the columns of the input";
    case hl::RowRefusal::step: return "a row's step is outside 2^26 .. 2^38 (1/64 .. 64 input items per output item)";
    case hl::RowRefusal::items: return "a row's length plus the taps per phase reaches 2^32";
    case hl::RowRefusal::phase: return "a row's phase0 is 2^63 or more";
    case hl::RowRefusal::columns: return "more than 2^31 output columns";
    case hl::RowRefusal::stride: return "a row stride below the column count";
    case hl::RowRefusal::lengths: return "no out_lengths array";
    case hl::RowRefusal::output: return "no output array";
    case hl::RowRefusal::input: return "no input array";
    default: return "";
    }
}

gr4pm_status refusal_status(const hl::RowPlan& p)
{
    switch (p.why) {
    case hl::RowRefusal::none:
    case hl::RowRefusal::nothing: return GR4PM_OK;
    case hl::RowRefusal::items:
    case hl::RowRefusal::phase:
    case hl::RowRefusal::columns:
        set_error("row_resampler: row %zu: %s", p.at, refusal_text(p.why));
        return GR4PM_ERR_OVERFLOW;
    default: set_error("row_resampler: row %zu: %s", p.at, refusal_text(p.why)); return GR4PM_ERR_INVALID;
    }
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
    GR4PM_TRY(design(phases, taps_per_phase, max_step, passband, stopband, h));
    for (size_t t = 0; t < h.size(); ++t) out[t] = static_cast<float>(h[t]);
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_row_resampler_create(const gr4pm_row_resampler_params* p, gr4pm_row_resampler** out)
try {
    if (!p || !out) return GR4PM_ERR_INVALID;
    *out = nullptr;
    const size_t Q = p->phases, P = p->taps_per_phase ? p->taps_per_phase : (p->taps ? 0 : 12);
    if (!sizes_or_error("row_resampler", Q, P)) return GR4PM_ERR_INVALID;
    std::vector<float> taps(Q * P + 1, 0.0f); // h[Q P] = 0
    if (p->taps) {
        std::copy(p->taps, p->taps + Q * P, taps.begin());
    } else {
        std::vector<double> h;
        GR4PM_TRY(design(Q, P, 1.0, 0.25, 0.75, h));
        for (size_t t = 0; t < h.size(); ++t) taps[t] = static_cast<float>(h[t]);
    }
    for (size_t t = 0; t < Q * P; ++t)
        if (!std::isfinite(taps[t])) {
            set_error("row_resampler: taps[%zu] is not finite", t);
            return GR4PM_ERR_INVALID;
        }
    GR4PM_TRY(require_device());
    std::unique_ptr<gr4pm_row_resampler> h(new (std::nothrow) gr4pm_row_resampler);
    if (!h) return GR4PM_ERR_NOMEM;
    h->Q = static_cast<uint32_t>(Q), h->P = static_cast<uint32_t>(P);
    h->stream = static_cast<hipStream_t>(p->stream);
    std::vector<float2> tab(Q * P);
    for (size_t s = 0; s < P; ++s)
        for (size_t q = 0; q < Q; ++q) {
            const size_t t = s * Q + q;
            const double d = static_cast<double>(taps[t + 1]) - static_cast<double>(taps[t]);
            tab[t] = float2{taps[t], static_cast<float>(d)};
        }
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
    GR4PM_TRY(refusal_status(p));
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
    GR4PM_TRY(refusal_status(p));
    if (p.why == hl::RowRefusal::nothing) {
        if (out_lengths && rows && n_rows <= hl::kRowMaxRows)
            for (size_t r = 0; r < n_rows; ++r) out_lengths[r] = 0; // no column
        return GR4PM_OK;
    }
    RowArgs a = {};
    a.x = reinterpret_cast<const float2*>(x), a.out = reinterpret_cast<float2*>(out), a.tab = h->d_tab.p;
    a.stride = stride, a.out_stride = out_stride;
    a.n_cols_out = static_cast<uint32_t>(n_cols_out);
    a.Q = h->Q, a.P = h->P, a.b = 32 - hl::row_log2(h->Q), a.T = p.T;
    for (size_t r = 0; r < n_rows; ++r) {
        a.n[r] = p.n[r], a.M[r] = p.M[r], a.rec[r] = rows[r];
        out_lengths[r] = p.M[r];
    }
    // the tables and the span a tile of T items can have at the call's largest step (row_tile() keeps it within the stage)
    uint64_t max_step = 0;
    for (size_t r = 0; r < n_rows; ++r) max_step = std::max(max_step, rows[r].step);
    const size_t smem = (static_cast<size_t>(h->Q) * h->P + hl::row_span_bound(p.T, max_step, h->P)) * sizeof(float2);
    hipLaunchKernelGGL(k_row_resample, dim3(p.grid_x, p.grid_y), dim3(hl::kRowThreads), smem, h->stream, a);
    GR4PM_HIP_TRY(hipGetLastError());
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

} // extern "C"
