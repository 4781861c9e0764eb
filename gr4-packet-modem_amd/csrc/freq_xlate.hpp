// freq_xlate.hpp -- what the Ddc (ddc.hip) and the Duc (duc.hip) share: the frequency word and create()'s checks of
// the frequencies, the rotated-tap table's entries and the complex multiply-accumulate of their definitions
// (include/gr4pm_hip.h).
#pragma once
#include "common.hpp"

#include <cmath>
#include <cstdint>

namespace gr4pm {

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

// ceil(2^32 / n) for n >= 2: j div n = umulhi(j, reciprocal_word(n)) for j < 2^13
inline unsigned reciprocal_word(size_t n) { return n >= 2 ? static_cast<unsigned>(((uint64_t(1) << 32) + n - 1) / n) : 0u; }

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
