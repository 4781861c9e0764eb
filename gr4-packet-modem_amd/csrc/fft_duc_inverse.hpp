// fft_duc_inverse.hpp -- the FftDuc's second kernel (fft_duc.hip has the description), templated on the output format, and
// its arguments.  fft_duc.hip instantiates it for complex64 and fft_duc_iq.hip for sc16 / sc8 / cu8 (DESIGN.md section
// 31): with the integer instantiations in a unit of their own, the complex64 kernel is compiled in the company it always
// had and comes out as it always did.  Both units are built with FFT_FLAGS.
#pragma once
#include "spectrum_segment.hpp"
#include "iq_format.hpp"

#include <type_traits>

namespace gr4pm {

struct InvArgs {
    const cf* spec; // [segments of the launch][2048]
    const float4* tT;
    const cf* cc;
    cf* out;        // the call's samples; of an integer format: its items, aligned to the item only
    size_t seg0;    // the launch's first segment, counted from the call's
    uint32_t n_seg; // segments of the launch
    uint32_t run;   // per wave
    uint32_t hop, V;
};

// what an integer instantiation takes: the complex64 one keeps InvArgs, the argument it always had
struct InvArgsIq : InvArgs {
    float gain;
    unsigned long long* clipped; // null, or the caller's device counter
};
template <int F>
using InvArgsFor = std::conditional_t<F == iq::kC64, InvArgs, InvArgsIq>;

// the integer instantiations' launch (fft_duc_iq.hip); format: GR4PM_IQ_SC16, _SC8 or _CU8
void fft_duc_launch_inverse_iq(dim3 grid, hipStream_t stream, const InvArgsIq& b, int format);

namespace { // internal linkage: one copy per unit, of the instantiations that unit asks for

// F: the output format, iq::kC64 for complex64.  An integer instantiation packs the sample where the complex64 one stores
// it (a.out counts its items) and has the clipped count to deliver: its waves without a segment stay to the end, and
// behind one more barrier the workgroup adds its total
template <int F>
__global__ __launch_bounds__(kW64Threads, 2) void k_fft_duc_inverse(InvArgsFor<F> a)
{
    __shared__ float4 lds4[kW64LdsF4]; // twiddles | eight exchange buffers
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < kW64TwFloat4; i += kW64Threads) lds4[i] = a.tT[i];
    __syncthreads(); // the only workgroup-wide synchronisation of the complex64 form; an integer one has a second, at its end
    float4* xb4 = lds4 + kW64TwFloat4 + wave * kW64BufF4;
    const uint32_t base = __builtin_amdgcn_readfirstlane(
        static_cast<uint32_t>(reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) char*)xb4)));
    const float4* row = xb4 + (lane & 31) * (kW64Row / 4);
    const float4* ldsT = lds4;
    const cf c = a.cc[lane];

    const uint32_t w = blockIdx.x * kW64Waves + wave;
    const uint64_t first = static_cast<uint64_t>(w) * a.run;
    constexpr bool kPack = F != iq::kC64;
    if (!kPack && first >= a.n_seg) return;
    const uint32_t count = kPack && first >= a.n_seg ? 0u : a.n_seg - first < a.run ? static_cast<uint32_t>(a.n_seg - first) : a.run;
    // An integer instantiation counts the wave's clipped components in a pad word of its own exchange buffer, which no
    // transform reads or writes (row 0, behind re[64] | im[64]): not a byte of LDS more (the kernel's budget is exact), and
    // no register that lives through the transforms
    constexpr int kPadDword = 128;
    static_assert(kPadDword >= 2 * 64 && kPadDword < kW64Row, "the count must sit in the pad of exchange row 0");
    uint32_t* const counts = reinterpret_cast<uint32_t*>(lds4 + kW64TwFloat4) + kPadDword; // wave w's at w kW64BufDwords
    if (kPack && lane == 0) counts[wave * kW64BufDwords] = 0;

    // half h of the launch's segment `seg`: bins lane + 64 j, j = 16 h .. 16 h + 15, real and imaginary parts swapped
    auto load_half = [&](cf* dst, uint64_t seg, int h) {
        const cf* x = a.spec + seg * kFftN + lane;
#pragma unroll
        for (int j = 16 * h; j < 16 * h + 16; ++j) dst[j] = swap_xy(x[64 * j]);
    };

    cf X[32];
    if (!kPack || count) {
        load_half(X, first, 0);
        load_half(X, first, 1);
    }
    for (uint32_t s = 0; s < count; ++s) {
        cf bq[32];
        dft32(X);
        w64_store(X, base);
        w64_mid_dev<1, true>(lane, row, ldsT, c, bq);
        const bool has_next = s + 1 < count;
        if (has_next) load_half(X, first + s + 1, 0);
        dft32(bq);
#pragma unroll
        for (int k = 0; k < 32; k += 4) w64_pin4(bq + k);
        if (has_next) load_half(X, first + s + 1, 1);
        // sample p = lane + 64 j of the segment is out[(seg0 + first + s) hop + p - V] for p >= V
        // (one address per lane, formed in integers: it lies in front of `out` for the lanes of segment 0 that store nothing
        // at small j)
        const int64_t at = static_cast<int64_t>((a.seg0 + first + s) * a.hop + lane) - static_cast<int64_t>(a.V);
        if constexpr (kPack) {
            // an item per lane: a wave instruction writes 64 consecutive items, 256 bytes of sc16 or 128 of sc8 / cu8, at
            // whatever multiple of the item the segment starts
            constexpr int64_t IB = iq::Fmt<F>::item_bytes;
            void* o = reinterpret_cast<void*>(reinterpret_cast<intptr_t>(a.out) + at * IB);
            // p >= V as j >= keep_from, the lane's first register that is kept, made afresh in every segment: the 32 lane
            // masks are the same for all segments, and hoisted out of the loop they take the scalar registers and spill
            // into a vector one; the kernel has none to spare beside the transform (192, tools/check_occupancy.py)
            uint32_t l = static_cast<uint32_t>(lane);
            asm volatile("" : "+v"(l));
            uint32_t keep_from = (a.V + 63u - l) >> 6;
            asm volatile("" : "+v"(keep_from)); // (and compared as it stands, with j: 32 shifted constants would take registers too)
            unsigned lane_clip = 0;
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                if (static_cast<uint32_t>(j) >= keep_from) // (x, y) swapped back, as the complex64 store has them
                    iq::put_item<F>(o, 64 * j, iq::pack_item<F, true>(float2{bq[j].y, bq[j].x}, a.gain, lane_clip)); // true: FFT_FLAGS
            }
            if (lane_clip) atomicAdd(&counts[wave * kW64BufDwords], lane_clip); // (LDS; rare: nothing clips at a sane gain)
        } else {
            cf* o = reinterpret_cast<cf*>(reinterpret_cast<intptr_t>(a.out) + at * static_cast<int64_t>(sizeof(cf)));
#pragma unroll
            for (int j = 0; j < 32; ++j)
                if (static_cast<uint32_t>(lane + 64 * j) >= a.V) o[64 * j] = swap_xy(bq[j]);
        }
    }
    if constexpr (kPack) {
        // the waves' counts, behind the kernel's second barrier: one atomic for the workgroup
        if (!a.clipped) return; // (the same in every thread)
        __syncthreads();
        if (tid == 0) {
            unsigned total = 0;
#pragma unroll
            for (int w = 0; w < kW64Waves; ++w) total += counts[w * kW64BufDwords];
            if (total) atomicAdd(a.clipped, static_cast<unsigned long long>(total));
        }
    }
}

} // namespace
} // namespace gr4pm
