// iq_format.hpp -- the integer IQ formats of include/gr4pm_hip.h (gr4pm_iq_format) as device code: one item's
// unpack and pack, shared by the converters (iq_format.hip), the integer ingest of the blocks that read a stream and the
// integer output of the Duc and the FftDuc.  Every float operation rounds on its own.  Unpacking is one product, in
// which there is nothing to contract; packing has a product and (cu8) a sum, and keeps them apart itself: both give the
// converters' bits under EXACT_FLAGS and under FFT_FLAGS.
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

// one component: x gain (+ 127.5 for cu8), to the nearest integer with ties to even, clamped; NaN: 0 (cu8: 128).
// The product and the sum round on their own whatever the file's flags: fft_duc_iq.hip packs under FFT_FLAGS
// (-ffp-contract=fast), where they fuse into one fma and cu8's byte differs in about two components per million at a
// gain that is no power of two.  That mode does not honour "#pragma clang fp contract(off)" and __fmul_rn is a plain
// product, so a caller in such a unit says kContracting = true and the product passes through an empty asm statement,
// which the optimiser cannot look through and which costs no instruction.  Units built with EXACT_FLAGS leave it false
// and compile to what they always did (the statement would reorder k_iq_pack's code)
template <int F, bool kContracting = false>
__device__ __forceinline__ uint32_t pack_component(float x, float gain, unsigned& clipped)
{
    float t = x * gain;
    if constexpr (F == GR4PM_IQ_CU8) {
        if constexpr (kContracting) asm("" : "+v"(t));
        t = t + Fmt<F>::bias;
    }
    const float r = rintf(t);
    const bool nan = t != t;
    const bool clip = nan || r < Fmt<F>::lo || r > Fmt<F>::hi;
    clipped += clip ? 1u : 0u;
    const float c = nan ? Fmt<F>::nan_value : fminf(fmaxf(r, Fmt<F>::lo), Fmt<F>::hi);
    constexpr uint32_t mask = Fmt<F>::item_bytes == 4 ? 0xFFFFu : 0xFFu;
    return static_cast<uint32_t>(static_cast<int>(c)) & mask;
}

// the item's bytes in the low bits of a word, as load_item() reads them
template <int F, bool kContracting = false>
__device__ __forceinline__ uint32_t pack_item(float2 x, float gain, unsigned& clipped)
{
    constexpr int cb = Fmt<F>::item_bytes * 4;
    const uint32_t i = pack_component<F, kContracting>(x.x, gain, clipped);
    const uint32_t q = pack_component<F, kContracting>(x.y, gain, clipped);
    return i | (q << cb);
}

// What a kernel templated on its OUTPUT format takes behind its other parameters (the Duc's and the FftDuc's kernels,
// DESIGN.md section 31): nothing for complex64, so that those instantiations read the arguments they always read
template <int F>
struct Out {
    float gain;
    unsigned long long* clipped; // null, or the caller's device counter
};
template <>
struct Out<kC64> {};

// item i of a stream that is written: pack_item()'s word, its low 4 or 2 bytes
template <int F>
__device__ __forceinline__ void put_item(void* p, size_t i, uint32_t w)
{
    if constexpr (Fmt<F>::item_bytes == 4)
        static_cast<uint32_t*>(p)[i] = w;
    else
        static_cast<uint16_t*>(p)[i] = static_cast<uint16_t>(w);
}

// the sum of a wave's per-lane counts, in lane 0
__device__ __forceinline__ unsigned wave_clipped(unsigned clip)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) clip += __shfl_down(clip, d, 64);
    return clip;
}

// gr4pm_iq_pack's count for a kernel that packs as it stores: the lanes' counts summed in the wave and, through NW
// words of LDS, in the workgroup, which adds its total with one atomic if anything clipped.  Every thread of the
// workgroup's NW waves comes here, behind its last store.  s_clip: NW words of the kernel's own LDS that nobody reads
// or writes any more (a stage that the last barrier has retired), so the count costs no LDS of its own
template <int NW>
__device__ __forceinline__ void add_clipped(unsigned clip, unsigned long long* counter, unsigned* s_clip)
{
    if (!counter) return; // (the same in every thread)
    clip = wave_clipped(clip);
    if ((threadIdx.x & 63) == 0) s_clip[threadIdx.x >> 6] = clip;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned total = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) total += s_clip[w];
        if (total) atomicAdd(counter, static_cast<unsigned long long>(total));
    }
}

} // namespace gr4pm::iq
