// row_kernel.hpp -- what the RowResampler (row_resampler.hip) and the StreamRowResampler (row_stream.hip) share: the
// one device body that k_row_resample and k_row_stream instantiate, with the per-row record it works on, the prototype
// design, the handle's coefficient table and the words of a refused call.  DESIGN.md sections 24 and 29.
//
// One body.  A one-shot call is a stream call on a fresh row: row_stream_start() with start = 0 gives d = phase0,
// ref_frac = 0 and Phi = -freq, so Phi + row_theta(freq, pos + 2^32) = row_theta(freq, pos) (the integer part gains freq,
// the fraction is untouched; pos + 2^32 stays in 64 bits since n + P - 1 < 2^32), and a fresh row's history is +0, which
// is what the one-shot call stages in front of a row.  tests/hostlogic/row_stream_plan_check.cpp sweeps both.  So the
// body works on the carried row's record (RowItem) on both sides, and an argument block that says it is not carried only
// takes out what a fresh row makes constant: that instantiation loads no history and passes the position to the rotator
// as it is.  The one-shot block's argument block makes the RowItem from the narrower records its calls bring (with the
// stream's 40-byte records in its arguments the one-shot call of 64 rows of 4096 items was 1.3 % slower at step 2.27,
// profiles/row_resampler_bench.txt).
//
// row_body: blockIdx.y is the row, blockIdx.x a tile of T output items of this call (T <= 1024, picked by the host from
//   the call's largest step so that the tile's input span fits the stage).  The row's record and the tile's first
//   position are wave-uniform; positions are relative to the call's first input item.  The workgroup copies the handle's
//   coefficient table and the tile's input span to LDS once: stage items in front of the call's first input item read
//   the row's history buffer (its last P - 1 items) where the row is carried and are +0 where it is not, the rest read
//   x_r, and an index at or behind the row's length is staged as +0 by an explicit range test and never loaded.  Lanes
//   then take consecutive output items, four per thread at the full tile.  Each lane has its own branch q and fraction
//   alpha, so the coefficients are per-lane LDS reads: one 8-byte read of {H, Dh}[s][q] and one of the sample per tap,
//   three fmaf.  The table is laid out [s][q], q fastest, the pair {H, Dh} in one float2: the ds_read_b64 of a tap takes
//   the bank pair q mod 32 in a half-wave of 32 lanes, so for Q <= 32 any pattern of q is conflict-free (equal q is one
//   address and broadcasts); Q = 64 .. 256 can put q and q + 32 k on one bank pair.  [q][s] with P = 12 would leave 12 q
//   mod 32 only eight bank pairs.  A tile wholly at or behind the row's count stores zeros and stages nothing.
// Nothing depends on the tile an item falls in or on the rows beside it.  Built with EXACT_FLAGS: every fmaf is written
// out, nothing else contracts.
#pragma once
#include "freq_xlate.hpp"
#include "hostlogic/row_stream_plan.hpp"
#include "kaiser_design.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace gr4pm {

struct RowItem { // 40 bytes: 64 of them and the header stay well inside the 4 KiB of kernel arguments
    uint64_t d, step; // the position of the call's first output item relative to its first input item, and the step
    int32_t freq;
    uint32_t phi, ref_frac;
    uint32_t n, M; // the call's input and output items
    uint32_t hist; // the buffer that holds the history the call reads
};

// An argument block of row_body has x, out, tab, stride, out_stride, n_cols_out, Q, P, b, T, `carried`, items_out(r) and
// item(r).  This is the stream's; the one-shot block's, with the narrower records its calls bring, is in row_resampler.hip.
struct RowArgs {
    static constexpr bool carried = true;
    const float2* x;
    float2* out;
    const float2* tab; // [P][Q] of {H[q][s], Dh[q][s]}
    float2* hist;      // [2][R][P - 1]
    size_t stride, out_stride;
    uint32_t n_cols_out;
    uint32_t Q, P, b, T, R;
    RowItem row[hostlogic::kRowMaxRows];
    __device__ uint32_t items_out(uint32_t r) const { return row[r].M; }
    __device__ RowItem item(uint32_t r) const { return row[r]; }
};
static_assert(sizeof(RowArgs) <= 4096, "the argument block");

__device__ __forceinline__ float2* history_of(const RowArgs& a, uint32_t buf, uint32_t r)
{
    return a.hist + (static_cast<size_t>(buf) * a.R + r) * (a.P - 1);
}

template <typename Args>
__device__ __forceinline__ void row_body(const Args& a, float2* s_row)
{
    namespace hl = hostlogic;
    constexpr bool Carried = Args::carried;
    const uint32_t tid = threadIdx.x;
    const uint32_t Q = a.Q, P = a.P, T = a.T, r = blockIdx.y;
    const uint32_t m0 = blockIdx.x * T; // below n_cols_out <= 2^31
    const uint32_t nv = hl::row_tile_items(m0, a.items_out(r), T);
    float2* __restrict__ row = a.out + static_cast<size_t>(r) * a.out_stride;
    if (nv == 0) { // wholly at or behind the call's count
        for (uint32_t m = tid; m < T && m0 + m < a.n_cols_out; m += hl::kRowThreads) row[m0 + m] = float2{0.0f, 0.0f};
        return;
    }
    const RowItem rec = a.item(r);
    const uint64_t n = rec.n;
    float2* tab = s_row;
    float2* st = s_row + Q * P;
    for (uint32_t i = tid; i < Q * P; i += hl::kRowThreads) tab[i] = a.tab[i];
    // stage item j is the item i0 - (P - 1) + j from the call's first: the tile's first item takes its oldest sample from j = 0
    const uint64_t pos0 = rec.d + static_cast<uint64_t>(m0) * rec.step;
    const uint64_t i0 = pos0 >> 32;
    const int64_t base = static_cast<int64_t>(i0) - static_cast<int64_t>(P - 1);
    const uint32_t S = static_cast<uint32_t>(hl::row_tile_span(pos0, nv, rec.step, P));
    const float2* __restrict__ xr = a.x + static_cast<size_t>(r) * a.stride;
    const float2* __restrict__ hr = nullptr;
    if constexpr (Carried) hr = history_of(a, rec.hist, r);
    for (uint32_t j = tid; j < S; j += hl::kRowThreads) {
        const int64_t k = base + j;
        float2 v = {0.0f, 0.0f};
        const hl::RowStreamSource from = hl::row_stream_source(k, n);
        if (from == hl::RowStreamSource::input)
            v = xr[k];
        else if (Carried && from == hl::RowStreamSource::history)
            v = hr[static_cast<int64_t>(P - 1) + k];
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
            const uint32_t theta = Carried ? rec.phi + hl::row_theta(rec.freq, hl::row_stream_theta_pos(pos, rec.ref_frac))
                                           : hl::row_theta(rec.freq, pos);
            cmac(y, mixer<-1>(theta, 1u), acc);
        }
        row[m0 + m] = y;
    }
}

inline bool row_sizes_or_error(const char* what, size_t Q, size_t P)
{
    if (hostlogic::row_sizes_valid(Q, P)) return true;
    set_error("%s: %zu phases of %zu taps: the phases are a power of two in [%u, %u], and there are 1 .. %zu taps in all", what, Q,
              P, hostlogic::kRowMinPhases, hostlogic::kRowMaxPhases, hostlogic::kRowMaxTaps);
    return false;
}

// gr4pm_row_resampler_taps: Q phases of ceil(per max(1, max_step)) taps, in double
inline gr4pm_status row_design(size_t Q, size_t per, double max_step, double passband, double stopband, std::vector<double>& h)
{
    if (!(max_step >= 1.0 / 64.0 && max_step <= 64.0)) { // a NaN fails
        set_error("row_resampler: max_step is %g, need 1/64 .. 64 input items per output item", max_step);
        return GR4PM_ERR_INVALID;
    }
    if (per < 1 || per > hostlogic::kRowMaxTaps) {
        set_error("row_resampler: %zu taps per phase, need 1 .. %zu / phases", per, hostlogic::kRowMaxTaps);
        return GR4PM_ERR_INVALID;
    }
    const double widen = std::max(1.0, max_step);
    const double span = std::ceil(static_cast<double>(per) * widen); // at most 4096 * 64
    if (!row_sizes_or_error("row_resampler", Q, static_cast<size_t>(span))) return GR4PM_ERR_INVALID;
    if (!(passband >= 0.0 && passband < stopband && passband + stopband <= 1.0)) {
        set_error("row_resampler: need 0 <= passband < stopband (units of the lower of the input and the output rate) and a "
                  "cutoff of at most half of it: passband + stopband <= 1");
        return GR4PM_ERR_INVALID;
    }
    const size_t P = static_cast<size_t>(span);
    kaiser_lowpass(Q * P, Q, passband / widen, stopband / widen, h, static_cast<double>(Q));
    return GR4PM_OK;
}

// a create()'s table for `phases` phases of `taps_per_phase` taps (0: 12 of the default design, or none with taps
// given): the sizes' check, the given taps or the design as floats, all finite, and {H, Dh}[s][q] with Dh the
// difference to the next tap in double (h[Q P] = 0)
inline gr4pm_status row_table(const char* what, size_t phases, size_t taps_per_phase, const float* given, uint32_t& Q_out,
                              uint32_t& P_out, std::vector<float2>& tab)
{
    const size_t Q = phases, P = taps_per_phase ? taps_per_phase : (given ? 0 : 12);
    if (!row_sizes_or_error(what, Q, P)) return GR4PM_ERR_INVALID;
    std::vector<float> taps(Q * P + 1, 0.0f);
    if (given) {
        std::copy(given, given + Q * P, taps.begin());
    } else {
        std::vector<double> h;
        GR4PM_TRY(row_design(Q, P, 1.0, 0.25, 0.75, h));
        for (size_t t = 0; t < h.size(); ++t) taps[t] = static_cast<float>(h[t]);
    }
    for (size_t t = 0; t < Q * P; ++t)
        if (!std::isfinite(taps[t])) {
            set_error("%s: taps[%zu] is not finite", what, t);
            return GR4PM_ERR_INVALID;
        }
    tab.resize(Q * P);
    for (size_t s = 0; s < P; ++s)
        for (size_t q = 0; q < Q; ++q) {
            const size_t t = s * Q + q;
            const double d = static_cast<double>(taps[t + 1]) - static_cast<double>(taps[t]);
            tab[t] = float2{taps[t], static_cast<float>(d)};
        }
    Q_out = static_cast<uint32_t>(Q), P_out = static_cast<uint32_t>(P);
    return GR4PM_OK;
}

// a refused call in words: "a row" where the call brings the rows' records, "the row" where the handle holds them
inline const char* row_refusal_text(hostlogic::RowRefusal why, bool carried)
{
    using hostlogic::RowRefusal;
    switch (why) {
    case RowRefusal::rows: return "at most 64 rows go into one call";
    case RowRefusal::records: return "no array of row records";
    case RowRefusal::length: return carried ? "the row's length exceeds the columns of the input" : "a row's length exceeds the columns of the input";
    case RowRefusal::step: return "a row's step is outside 2^26 .. 2^38 (1/64 .. 64 input items per output item)";
    case RowRefusal::items:
        return carried ? "the row's length plus the taps per phase reaches 2^32" : "a row's length plus the taps per phase reaches 2^32";
    case RowRefusal::phase: return "a row's phase0 is 2^63 or more";
    case RowRefusal::columns: return "more than 2^31 output columns";
    case RowRefusal::stride: return "a row stride below the column count";
    case RowRefusal::lengths: return "no out_lengths array";
    case RowRefusal::room: return "the row makes more items in this call than the output has columns; a stream loses none";
    case RowRefusal::output: return "no output array";
    case RowRefusal::input: return "no input array";
    default: return "";
    }
}

// the status of a plan's `why`, with the error text where it refuses
inline gr4pm_status row_refusal_status(hostlogic::RowRefusal why, size_t at, bool carried)
{
    using hostlogic::RowRefusal;
    if (why == RowRefusal::none || why == RowRefusal::nothing) return GR4PM_OK;
    set_error("%s: row %zu: %s", carried ? "row_stream" : "row_resampler", at, row_refusal_text(why, carried));
    const bool overflow = why == RowRefusal::items || why == RowRefusal::phase || why == RowRefusal::columns || why == RowRefusal::room;
    return overflow ? GR4PM_ERR_OVERFLOW : GR4PM_ERR_INVALID;
}

} // namespace gr4pm
