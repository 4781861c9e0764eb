// freq_xlate.hpp -- what the Ddc (ddc.hip) and the Duc (duc.hip) share: the frequency word and create()'s checks of
// its arguments, the rotated-tap table's entries, the complex multiply-accumulate of their definitions
// (include/gr4pm_hip.h) and the fragments their four kernels have in common: the dispatch on a workgroup's channel
// count, the mixer's phasor, the stage laid out by phase and the tile that leaves as 16-byte stores.  The tiles'
// sizes are hostlogic/xlate_geometry.hpp's.
#pragma once
#include "common.hpp"
#include "hostlogic/xlate_geometry.hpp"
#include "iq_format.hpp"

#include <cmath>
#include <cstdint>
#include <type_traits>

namespace gr4pm {

using hostlogic::kNt;

typedef const float __attribute__((address_space(4))) * ConstTaps; // a table written at create only, float by float:
                                                                    // a wave-uniform address there is a scalar load

// fn(std::integral_constant<int, NC>) for the NC = min(left, 8) channels of a workgroup, left >= 1
template <typename Fn>
__device__ __forceinline__ void with_channels(unsigned left, Fn&& fn)
{
    switch (left < 8 ? left : 8) {
    case 1: fn(std::integral_constant<int, 1>{}); break;
    case 2: fn(std::integral_constant<int, 2>{}); break;
    case 3: fn(std::integral_constant<int, 3>{}); break;
    case 4: fn(std::integral_constant<int, 4>{}); break;
    case 5: fn(std::integral_constant<int, 5>{}); break;
    case 6: fn(std::integral_constant<int, 6>{}); break;
    case 7: fn(std::integral_constant<int, 7>{}); break;
    default: fn(std::integral_constant<int, 8>{}); break;
    }
}

// exp(Sign 2 pi j phi / 2^32) for phi = (w i) mod 2^32: double sincospi of Sign phi / 2^31, an exact argument,
// rounded to float
template <int Sign>
__device__ __forceinline__ float2 mixer(uint32_t w, uint32_t i)
{
    const uint32_t phi = w * i;
    const double turn = static_cast<double>(phi);
    double sn, cs;
    sincospi((Sign < 0 ? -turn : turn) * (1.0 / 2147483648.0), &sn, &cs);
    return float2{static_cast<float>(cs), static_cast<float>(sn)};
}

// the stage by phase: item j of its S at row j mod D, column j div D, rows of RS items (odd), so that lanes D items
// apart read consecutive items of a row.  Item j is sample(v0 + j) of a virtual stream of `total` samples, zero beyond.
template <typename Sample>
__device__ __forceinline__ void stage_by_phase(float2* s, unsigned S, unsigned step, unsigned D, unsigned rcpD, unsigned RS,
                                               size_t v0, size_t total, Sample&& sample)
{
    for (unsigned j = threadIdx.x; j < S; j += step) {
        const unsigned col = D == 1 ? j : __umulhi(j, rcpD);
        const unsigned row = j - col * D;
        const size_t v = v0 + j;
        s[row * RS + col] = v < total ? sample(v) : float2{0.0f, 0.0f};
    }
}

// the same for a row without a format, hist[0 .. H) ++ in[0 ..), and a workgroup of kNt threads.  No lambda, and the
// sizes by reference so that a kernel's argument members are read where the loop uses them: through the overload
// above k_duc_rational comes to 714 instructions (the parent's has 709) and 64 VGPRs (63), through this one to 708 and 63
__device__ __forceinline__ void stage_by_phase(float2* s, const unsigned& S, const unsigned& D, const unsigned& rcpD,
                                               const unsigned& RS, size_t v0, const size_t& total, const float2* hist,
                                               unsigned H, const float2* in)
{
    for (unsigned j = threadIdx.x; j < S; j += kNt) {
        const unsigned col = D == 1 ? j : __umulhi(j, rcpD), row = j - col * D;
        const size_t v = v0 + j;
        float2 x = {0.0f, 0.0f};
        if (v < total) x = v < H ? hist[v] : in[v - H];
        s[row * RS + col] = x;
    }
}

// out[0 .. n) = sample(0 .. n) by the workgroup's kNt threads, two samples per 16-byte store from item `head` on:
// head = 1 where out is only 8-byte aligned, and item 0 leaves alone
template <typename Sample>
__device__ __forceinline__ void store_tile(float2* __restrict__ out, unsigned n, unsigned head, Sample&& sample)
{
    const unsigned tid = threadIdx.x;
    if (tid == 0 && head && n) out[0] = sample(0);
    for (unsigned t = head + 2 * tid; t < n; t += 2 * kNt) {
        if (t + 1 < n) {
            const float2 lo = sample(t), hi = sample(t + 1);
            *reinterpret_cast<float4*>(out + t) = float4{lo.x, lo.y, hi.x, hi.y};
        } else {
            out[t] = sample(t);
        }
    }
}

// the same tile as integer IQ: items 0 .. n of format F at `out`, item t = pack_item(sample(t)), by the workgroup's kNt
// threads.  A lane packs the two samples it would have stored as complex64 (the same tile reads) and stores them as one
// word pair (sc16: 8 bytes) or one word (sc8, cu8: 4 bytes), so a wave instruction writes 512 or 256 contiguous bytes.
// `out` is aligned to its item only: where it is not aligned to the pair, item 0 leaves alone (head = 1), and the pairs
// behind it are aligned
template <int F, typename Sample>
__device__ __forceinline__ void store_tile_iq(unsigned char* __restrict__ out, unsigned n, float gain, unsigned& clipped, Sample&& sample)
{
    constexpr unsigned IB = iq::Fmt<F>::item_bytes;
    const unsigned tid = threadIdx.x;
    const unsigned head = static_cast<unsigned>(reinterpret_cast<uintptr_t>(out) / IB) & 1u;
    if (tid == 0 && head && n) iq::put_item<F>(out, 0, iq::pack_item<F>(sample(0), gain, clipped));
    for (unsigned t = head + 2 * tid; t < n; t += 2 * kNt) {
        const uint32_t lo = iq::pack_item<F>(sample(t), gain, clipped);
        if (t + 1 < n) {
            const uint32_t hi = iq::pack_item<F>(sample(t + 1), gain, clipped);
            if constexpr (IB == 4)
                *reinterpret_cast<uint2*>(out + static_cast<size_t>(t) * IB) = uint2{lo, hi};
            else
                *reinterpret_cast<uint32_t*>(out + static_cast<size_t>(t) * IB) = lo | (hi << 16);
        } else {
            iq::put_item<F>(out, t, lo);
        }
    }
}

// acc += g x, each product and sum one fmaf, in this order
__device__ __forceinline__ void cmac(float2& acc, float2 g, float2 x)
{
    acc.x = fmaf(g.x, x.x, acc.x);
    acc.x = fmaf(-g.y, x.y, acc.x);
    acc.y = fmaf(g.x, x.y, acc.y);
    acc.y = fmaf(g.y, x.x, acc.y);
}

// llrint(f 2^32) mod 2^32: f = trunc(f) + m exactly, and trunc(f) 2^32 is a multiple of 2^32 that moves no tie
inline uint32_t frequency_word(double f)
{
    const double m = std::fmod(f, 1.0);
    return static_cast<uint32_t>(static_cast<uint64_t>(std::llrint(m * 4294967296.0)));
}

// a create()'s frequencies: 1 .. max_K of them, all finite, as words
inline gr4pm_status frequency_words(const char* name, const double* f, size_t K, size_t max_K, std::vector<uint32_t>& words)
{
    if (K < 1 || K > max_K) {
        set_error("%s: the number of channels must be in [1, %zu], not %zu", name, max_K, K);
        return GR4PM_ERR_INVALID;
    }
    if (!f) {
        set_error("%s: no frequencies", name);
        return GR4PM_ERR_INVALID;
    }
    words.resize(K);
    for (size_t k = 0; k < K; ++k) {
        if (!std::isfinite(f[k])) {
            set_error("%s: frequencies[%zu] is not finite", name, k);
            return GR4PM_ERR_INVALID;
        }
        words[k] = frequency_word(f[k]);
    }
    return GR4PM_OK;
}

// I and D within their ranges: what a tap design and a create() check alike
inline gr4pm_status ratio_ranges(const char* name, size_t I, size_t max_I, size_t D, size_t max_D)
{
    if (I < 1 || I > max_I) {
        set_error("%s: the interpolation must be in [1, %zu], not %zu", name, max_I, I);
        return GR4PM_ERR_INVALID;
    }
    if (D < 1 || D > max_D) {
        set_error("%s: the decimation must be in [1, %zu], not %zu", name, max_D, D);
        return GR4PM_ERR_INVALID;
    }
    return GR4PM_OK;
}

// the sizes of a tap design: the ratio's ranges, and 1 .. max_L taps at P per phase of `phases`: `per` names them, "a
// decimation" with the Ddc's D and "an interpolation" with the Duc's I
inline gr4pm_status design_sizes(const char* name, size_t I, size_t max_I, size_t D, size_t max_D, size_t P, size_t phases,
                                 const char* per, size_t max_L)
{
    GR4PM_TRY(ratio_ranges(name, I, max_I, D, max_D));
    if (P < 1 || P * phases > max_L) {
        set_error("%s: %zu taps per phase at %s of %zu: the prototype has 1 .. %zu taps", name, P, per, phases, max_L);
        return GR4PM_ERR_INVALID;
    }
    return GR4PM_OK;
}

// a create()'s ratio I / D: both within their ranges, and in lowest terms
inline gr4pm_status resample_ratio(const char* name, size_t I, size_t max_I, size_t D, size_t max_D)
{
    GR4PM_TRY(ratio_ranges(name, I, max_I, D, max_D));
    size_t gcd = I;
    for (size_t b = D % I; b;) {
        const size_t r = gcd % b;
        gcd = b, b = r;
    }
    if (gcd != 1) {
        set_error("%s: the ratio %zu / %zu is not in lowest terms: use %zu / %zu", name, I, D, I / gcd, D / gcd);
        return GR4PM_ERR_INVALID;
    }
    return GR4PM_OK;
}

// a create()'s cap on what one call may take or make
inline gr4pm_status per_call_cap(const char* name, const char* what, size_t n)
{
    if (n == 0 || n > (size_t(1) << 31)) {
        set_error("%s: %s must be in [1, 2^31]", name, what);
        return GR4PM_ERR_INVALID;
    }
    return GR4PM_OK;
}

// a create()'s own prototype, where it has one: 1 .. max_L taps
inline gr4pm_status prototype_length(const char* name, const float* taps, size_t n, size_t max_L)
{
    if (taps && (n < 1 || n > max_L)) {
        set_error("%s: the prototype has 1 .. %zu taps, not %zu", name, max_L, n);
        return GR4PM_ERR_INVALID;
    }
    return GR4PM_OK;
}

// a create()'s gains, where it has them: all finite
inline gr4pm_status finite_gains(const char* name, const double* gains, size_t K)
{
    for (size_t k = 0; gains && k < K; ++k)
        if (!std::isfinite(gains[k])) {
            set_error("%s: gains[%zu] is not finite", name, k);
            return GR4PM_ERR_INVALID;
        }
    return GR4PM_OK;
}

// w / 2^32 folded to [-0.5, 0.5)
inline double folded_frequency(uint32_t w)
{
    return (static_cast<double>(w) - (w >= 0x80000000u ? 4294967296.0 : 0.0)) / 4294967296.0;
}

// exp(2 pi j phi / 2^32) in double, exact at the multiples of pi / 2 (cos(pi / 2) in double is 6e-17, not 0)
inline void unit_phasor(uint32_t phi, double& c, double& s)
{
    const double ang = 0.5 * 3.14159265358979323846 * static_cast<double>(phi & 0x3FFFFFFFu) / 1073741824.0;
    const double c0 = std::cos(ang), s0 = std::sin(ang);
    switch (phi >> 30) {
    case 0: c = c0, s = s0; break;
    case 1: c = -s0, s = c0; break;
    case 2: c = -c0, s = -s0; break;
    default: c = s0, s = -c0; break;
    }
}

// one entry of a rotated-tap table: h exp(+2 pi j phi / 2^32), each component rounded to float once
inline float2 rotated_tap(double h, uint32_t phi)
{
    double c, s;
    unit_phasor(phi, c, s);
    return float2{static_cast<float>(h * c), static_cast<float>(h * s)};
}

} // namespace gr4pm
