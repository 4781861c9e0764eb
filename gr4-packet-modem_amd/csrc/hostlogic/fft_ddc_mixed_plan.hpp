// hostlogic/fft_ddc_mixed_plan.hpp -- the integer side of the MixedFftDdc block (fft_ddc.hip),
// HIP-free: the FftDdc's (fft_ddc_plan.hpp) with a decimation per channel.
//
// N = 2048, K channels; channel k has D_k, a power of two in 4 .. 64, B_k = N / D_k, L_k taps and R_k images.
// Dmax = max D_k.  One overlap V for the handle with Dmax | V, V <= N - 64 and, for every k,
//     V - (Dmax - D_k) >= L_k - 1,
// hop = N - V.  All channels share one segment grid, anchored on Dmax: segment s is the N items from
//     a_s = s hop - V + Dmax - 1
// on, which is fft_ddc_shape(Dmax, V) and fft_ddc_plan() unchanged.  Channel k keeps the items
//     n' = first_k .. first_k + frames_k - 1,   first_k = (V - Dmax) / D_k + 1,   frames_k = hop / D_k
// of its B_k-point inverse transform.  Frame n = s frames_k + n' - first_k has its newest sample at
// a_s + n' D_k = n D_k + D_k - 1, the Ddc's frame grid at D_k; the smallest kept item of the segment is
// p = first_k D_k = V - Dmax + D_k >= L_k - 1, beyond the circular wrap, and the largest is N - Dmax.
#pragma once
#include "fft_ddc_plan.hpp"

namespace gr4pm {
namespace hostlogic {

enum class FftDdcMixedRefusal { none, channels, decimation, images, taps, overlap_multiple, overlap_high, overlap_low };

// what was refused, and for the per-channel refusals the first channel it holds for
struct FftDdcMixedVerdict {
    FftDdcMixedRefusal refusal;
    size_t channel;
};

// everything that does not need the overlap: K, and per channel D_k, R_k and L_k
constexpr FftDdcMixedVerdict fft_ddc_mixed_validate_channels(size_t K, const size_t* D, const size_t* R, const size_t* L)
{
    if (K < 1 || K > kFftDdcMaxK) return {FftDdcMixedRefusal::channels, 0};
    for (size_t k = 0; k < K; ++k)
        if (!fft_ddc_pow2(D[k]) || D[k] < kFftDdcMinD || D[k] > kFftDdcMaxD) return {FftDdcMixedRefusal::decimation, k};
    for (size_t k = 0; k < K; ++k)
        if (!fft_ddc_pow2(R[k]) || R[k] > D[k]) return {FftDdcMixedRefusal::images, k};
    for (size_t k = 0; k < K; ++k)
        if (L[k] < 1) return {FftDdcMixedRefusal::taps, k};
    return {FftDdcMixedRefusal::none, 0};
}

// Dmax of decimations that fft_ddc_mixed_validate_channels() took
constexpr size_t fft_ddc_mixed_max_decimation(size_t K, const size_t* D)
{
    size_t m = 0;
    for (size_t k = 0; k < K; ++k) m = D[k] > m ? D[k] : m;
    return m;
}

// the smallest multiple of 256 that is >= max_k (Dmax - D_k + L_k - 1), for channels that were validated (L_k within a
// size_t's half); it may lie above N - 64, which fft_ddc_mixed_validate() then refuses
constexpr size_t fft_ddc_mixed_default_overlap(size_t K, const size_t* D, const size_t* L)
{
    const size_t Dmax = fft_ddc_mixed_max_decimation(K, D);
    size_t reach = 0;
    for (size_t k = 0; k < K; ++k) {
        const size_t r = Dmax - D[k] + L[k] - 1;
        reach = r > reach ? r : reach;
    }
    return (reach + 255) / 256 * 256;
}

constexpr FftDdcMixedVerdict fft_ddc_mixed_validate(size_t K, const size_t* D, const size_t* R, const size_t* L, size_t V)
{
    const FftDdcMixedVerdict v = fft_ddc_mixed_validate_channels(K, D, R, L);
    if (v.refusal != FftDdcMixedRefusal::none) return v;
    const size_t Dmax = fft_ddc_mixed_max_decimation(K, D);
    if (V % Dmax) return {FftDdcMixedRefusal::overlap_multiple, 0};
    if (V > kFftDdcN - kFftDdcMinHop) return {FftDdcMixedRefusal::overlap_high, 0};
    for (size_t k = 0; k < K; ++k) // V - (Dmax - D_k) >= L_k - 1, without a negative left side or a wrap
        if (V < Dmax - D[k] || V - (Dmax - D[k]) < L[k] - 1) return {FftDdcMixedRefusal::overlap_low, k};
    return {FftDdcMixedRefusal::none, 0};
}

// what Dmax, V and D_k fix for channel k
struct FftDdcMixedChannel {
    uint32_t first;  // (V - Dmax) / D_k + 1: the first n' that is kept
    uint32_t frames; // hop / D_k: frames of a segment
};

// V - Dmax + D_k is not negative for a validated handle (V = 0 needs D_k = Dmax) and a multiple of D_k
constexpr FftDdcMixedChannel fft_ddc_mixed_channel(uint32_t Dmax, uint32_t V, uint32_t D)
{
    return FftDdcMixedChannel{(V + D - Dmax) / D, (kFftDdcN - V) / D};
}

// the response tables lie behind one another in channel order, R_k B_k items each: offsets[k], and the total returned
constexpr size_t fft_ddc_mixed_table_offsets(size_t K, const size_t* D, const size_t* R, size_t* offsets)
{
    size_t at = 0;
    for (size_t k = 0; k < K; ++k) {
        offsets[k] = at;
        at += R[k] * (kFftDdcN / D[k]);
    }
    return at;
}

// frames of channel k in a call that fft_ddc_plan(fft_ddc_shape(Dmax, V), taken, n) describes
constexpr size_t fft_ddc_mixed_frames(const FftDdcPlan& p, const FftDdcMixedChannel& c) { return p.n_segments * c.frames; }

} // namespace hostlogic
} // namespace gr4pm
