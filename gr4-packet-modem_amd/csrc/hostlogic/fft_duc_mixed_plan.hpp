// hostlogic/fft_duc_mixed_plan.hpp -- the integer side of the MixedFftDuc block (fft_duc.hip),
// HIP-free: the FftDuc's (fft_duc_plan.hpp) with an interpolation per row.
//
// N = 2048, K rows; row k has I_k, a power of two in 4 .. 64, B_k = N / I_k, L_k taps and R_k images.  Imax = max I_k.
// One overlap V for the handle with Imax | V, V <= N - 64 and V >= L_k - 1 for every k, hop = N - V.  Row k's item m sits
// at output sample m I_k; all rows start at output sample 0.  Segment s is the N output samples from
//     a_s = s hop - V
// on, a multiple of Imax and so of every I_k: it is made of the B_k items m = a_s / I_k + n', n' = 0 .. B_k - 1, of row k.
//
// The handle counts in slots of Imax output samples: a call of u slots takes u Imax / I_k items of row k, and its plan is
// fft_duc_plan(fft_duc_shape(Imax, V), taken_slots, u) unchanged.  Per row only the factor Imax / I_k is new: row k carries
// H_k = (V + pending Imax) / I_k < B_k items between calls, and a segment completes hop / I_k of its items.  (Unlike the
// MixedFftDdc nothing like Dmax - D_k is charged to a fast row: the Duc's grid has no D - 1 offset, a_s itself is on
// every row's grid.)
#pragma once
#include "fft_duc_plan.hpp"

namespace gr4pm {
namespace hostlogic {

enum class FftDucMixedRefusal { none, channels, interpolation, images, taps, overlap_multiple, overlap_high, overlap_low };

// what was refused, and for the per-row refusals the first row it holds for
struct FftDucMixedVerdict {
    FftDucMixedRefusal refusal;
    size_t channel;
};

// everything that does not need the overlap: K, and per row I_k, R_k and L_k
constexpr FftDucMixedVerdict fft_duc_mixed_validate_channels(size_t K, const size_t* I, const size_t* R, const size_t* L)
{
    if (K < 1 || K > kFftDucMaxK) return {FftDucMixedRefusal::channels, 0};
    for (size_t k = 0; k < K; ++k)
        if (!fft_ddc_pow2(I[k]) || I[k] < kFftDucMinI || I[k] > kFftDucMaxI) return {FftDucMixedRefusal::interpolation, k};
    for (size_t k = 0; k < K; ++k)
        if (!fft_ddc_pow2(R[k]) || R[k] > I[k]) return {FftDucMixedRefusal::images, k};
    for (size_t k = 0; k < K; ++k)
        if (L[k] < 1) return {FftDucMixedRefusal::taps, k};
    return {FftDucMixedRefusal::none, 0};
}

// Imax of interpolations that fft_duc_mixed_validate_channels() took
constexpr size_t fft_duc_mixed_max_interpolation(size_t K, const size_t* I)
{
    size_t m = 0;
    for (size_t k = 0; k < K; ++k) m = I[k] > m ? I[k] : m;
    return m;
}

// the smallest multiple of 256 that is >= max_k (L_k - 1), for rows that were validated; it may lie above N - 64, which
// fft_duc_mixed_validate() then refuses
constexpr size_t fft_duc_mixed_default_overlap(size_t K, const size_t* L)
{
    size_t reach = 0;
    for (size_t k = 0; k < K; ++k) reach = L[k] - 1 > reach ? L[k] - 1 : reach;
    return (reach + 255) / 256 * 256;
}

constexpr FftDucMixedVerdict fft_duc_mixed_validate(size_t K, const size_t* I, const size_t* R, const size_t* L, size_t V)
{
    const FftDucMixedVerdict v = fft_duc_mixed_validate_channels(K, I, R, L);
    if (v.refusal != FftDucMixedRefusal::none) return v;
    if (V % fft_duc_mixed_max_interpolation(K, I)) return {FftDucMixedRefusal::overlap_multiple, 0};
    if (V > kFftDucN - kFftDucMinHop) return {FftDucMixedRefusal::overlap_high, 0};
    for (size_t k = 0; k < K; ++k)
        if (V < L[k] - 1) return {FftDucMixedRefusal::overlap_low, k};
    return {FftDucMixedRefusal::none, 0};
}

// what Imax, V and I_k fix for row k
struct FftDucMixedRow {
    uint32_t ratio;     // Imax / I_k: items of the row in a slot
    uint32_t hop_items; // hop / I_k: items of the row that complete a segment
    uint32_t keep;      // V / I_k: items of a segment in front of its hop_items new ones
};

constexpr FftDucMixedRow fft_duc_mixed_row(uint32_t Imax, uint32_t V, uint32_t I)
{
    return FftDucMixedRow{Imax / I, (kFftDucN - V) / I, V / I};
}

// of a call that p = fft_duc_plan(fft_duc_shape(Imax, V), taken_slots, slots) describes, for row r: the items it takes, the
// items in front of them (H_k) and the items it leaves behind
constexpr size_t fft_duc_mixed_items(const FftDucMixedRow& r, size_t slots) { return slots * r.ratio; }
constexpr size_t fft_duc_mixed_carried(const FftDucPlan& p, const FftDucMixedRow& r) { return p.carried * r.ratio; }
constexpr size_t fft_duc_mixed_left(const FftDucPlan& p, const FftDucMixedRow& r) { return p.left * r.ratio; }

// the slots of one call are bounded by 2^40 items in the row with the most items per slot
constexpr bool fft_duc_mixed_slots_fit(size_t slots, uint32_t max_ratio) { return slots <= (size_t(1) << 40) / max_ratio; }

// the response tables lie behind one another in row order, R_k B_k items each: offsets[k], and the total returned
constexpr size_t fft_duc_mixed_table_offsets(size_t K, const size_t* I, const size_t* R, size_t* offsets)
{
    size_t at = 0;
    for (size_t k = 0; k < K; ++k) {
        offsets[k] = at;
        at += R[k] * (kFftDucN / I[k]);
    }
    return at;
}

// the carried items lie behind one another in row order with room for B_k - 1 each (H_k < B_k): offsets[k], and the total
constexpr size_t fft_duc_mixed_carried_offsets(size_t K, const size_t* I, size_t* offsets)
{
    size_t at = 0;
    for (size_t k = 0; k < K; ++k) {
        offsets[k] = at;
        at += kFftDucN / I[k] - 1;
    }
    return at;
}

} // namespace hostlogic
} // namespace gr4pm
