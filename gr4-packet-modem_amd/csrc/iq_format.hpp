// iq_format.hpp -- the integer IQ formats of include/gr4pm_hip.h (gr4pm_iq_format) as device code: one item's
// unpack and pack, shared by the converters (iq_format.hip) and the channelizer's integer ingest (channelizer.hip).
// Every float operation rounds on its own: include from files built with EXACT_FLAGS only.
#pragma once
#include <cstdint>

#include "common.hpp"

namespace gr4pm::iq {

constexpr int kC64 = 0; // "no integer format": the complex64 instantiations of a kernel templated on the format

template <int F>
struct Fmt;
template <>
struct Fmt<GR4PM_IQ_SC16> {
    static constexpr int item_bytes = 4;
    static constexpr float lo = -32768.0f, hi = 32767.0f, bias = 0.0f, nan_value = 0.0f;
};
template <>
struct Fmt<GR4PM_IQ_SC8> {
    static constexpr int item_bytes = 2;
    static constexpr float lo = -128.0f, hi = 127.0f, bias = 0.0f, nan_value = 0.0f;
};
template <>
struct Fmt<GR4PM_IQ_CU8> {
    static constexpr int item_bytes = 2;
    static constexpr float lo = 0.0f, hi = 255.0f, bias = 127.5f, nan_value = 128.0f;
};

inline bool valid(int f) { return f == GR4PM_IQ_SC16 || f == GR4PM_IQ_SC8 || f == GR4PM_IQ_CU8; }
inline size_t item_bytes(int f) { return f == GR4PM_IQ_SC16 ? 4 : 2; }
inline float default_scale(int f) { return f == GR4PM_IQ_SC16 ? 1.0f / 32768.0f : 1.0f / 128.0f; }
inline float default_gain(int f) { return f == GR4PM_IQ_SC16 ? 32768.0f : 128.0f; }

// item i of a stream: its bytes, little-endian, in the low bits of a word
template <int F>
__device__ __forceinline__ uint32_t load_item(const void* p, size_t i)
{
    if constexpr (Fmt<F>::item_bytes == 4)
        return static_cast<const uint32_t*>(p)[i];
    else
        return static_cast<const uint16_t*>(p)[i];
}

template <int F>
__device__ __forceinline__ float component(uint32_t bits)
{
    if constexpr (F == GR4PM_IQ_SC16)
        return static_cast<float>(static_cast<int16_t>(bits));
    else if constexpr (F == GR4PM_IQ_SC8)
        return static_cast<float>(static_cast<int8_t>(bits));
    else
        return static_cast<float>(bits & 0xFFu) - 127.5f; // exact: a multiple of 0.5 below 2^8
}

// raw: load_item()'s word.  The conversion and the offset are exact, the product is the one rounding.
template <int F>
__device__ __forceinline__ float2 unpack_item(uint32_t raw, float scale)
{
    constexpr int cb = Fmt<F>::item_bytes * 4; // bits of a component
    return float2{component<F>(raw) * scale, component<F>(raw >> cb) * scale};
}

// one component: x gain (+ 127.5 for cu8), to the nearest integer with ties to even, clamped; NaN: 0 (cu8: 128)
template <int F>
__device__ __forceinline__ uint32_t pack_component(float x, float gain, unsigned& clipped)
{
    float t = x * gain;
    if constexpr (F == GR4PM_IQ_CU8) t = t + Fmt<F>::bias;
    const float r = rintf(t);
    const bool nan = t != t;
    const bool clip = nan || r < Fmt<F>::lo || r > Fmt<F>::hi;
    clipped += clip ? 1u : 0u;
    const float c = nan ? Fmt<F>::nan_value : fminf(fmaxf(r, Fmt<F>::lo), Fmt<F>::hi);
    constexpr uint32_t mask = Fmt<F>::item_bytes == 4 ? 0xFFFFu : 0xFFu;
    return static_cast<uint32_t>(static_cast<int>(c)) & mask;
}

// the item's bytes in the low bits of a word, as load_item() reads them
template <int F>
__device__ __forceinline__ uint32_t pack_item(float2 x, float gain, unsigned& clipped)
{
    constexpr int cb = Fmt<F>::item_bytes * 4;
    const uint32_t i = pack_component<F>(x.x, gain, clipped);
    const uint32_t q = pack_component<F>(x.y, gain, clipped);
    return i | (q << cb);
}

} // namespace gr4pm::iq
