// spectrum_segment.hpp -- what the Spectrum and the Spectrogram blocks share (spectrum.hip, spectrogram.hip): how a wave
// of the one-exchange transform loads half of a segment, and the part of create() that is the same for both: the window
// (the caller's or periodic Hann, checked, with its power), the transform's tables and the waves of one launch.
#pragma once
#include "stream_tail.hpp"
#include "correlate_w64.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace gr4pm {
namespace { // internal linkage, as stream_tail.hpp's kernel: one copy per unit

// Half h (0 or 1) of the segment that begins at item v0 of the virtual stream hist[0 .. H) ++ in[0 ..): register j of
// lane l takes item v0 + l + 64 j, j = 16 h .. 16 h + 15.  A segment that begins in the carried samples comes through
// iq::vsample(), any other straight from the input; an integer format converts right here.  The stream's values come
// by reference, as in iq::vsample(): a kernel's argument members are read where they are used.
template <int F>
__device__ __forceinline__ void load_half_segment(cf* dst, const float2* const& hist, const size_t& H, const void* const& in,
                                                  const float& scale, size_t v0, int lane, int h)
{
    int ln = lane;
    asm volatile("" : "+v"(ln)); // addresses are formed here, not hoisted out of the segment loop
    if (v0 >= H) { // uniform: the whole segment lies in the input
        const size_t i0 = v0 - H + ln;
        if constexpr (F == iq::kC64) {
            const cf* x = static_cast<const cf*>(in) + i0;
#pragma unroll
            for (int j = 16 * h; j < 16 * h + 16; ++j) dst[j] = x[64 * j];
        } else {
#pragma unroll
            for (int j = 16 * h; j < 16 * h + 16; ++j) {
                const float2 s = iq::unpack_item<F>(iq::load_item<F>(in, i0 + 64 * j), scale);
                dst[j] = mk(s.x, s.y);
            }
        }
    } else {
#pragma unroll
        for (int j = 16 * h; j < 16 * h + 16; ++j) {
            const float2 s = iq::vsample<F>(hist, H, in, scale, v0 + ln + 64 * j);
            dst[j] = mk(s.x, s.y);
        }
    }
}

inline void hann(uint32_t n, float* out)
{
    for (uint32_t i = 0; i < n; ++i)
        out[i] = static_cast<float>(0.5 - 0.5 * std::cos(2.0 * M_PI * static_cast<double>(i) / static_cast<double>(n)));
}

// the device side of a handle that transforms windowed segments of 2048 samples
struct SegmentTransform {
    double window_power = 0.0; // sum w[n]^2
    size_t max_waves = 2048;   // of one launch: eight per compute unit, at most 2048
    DevBuf<float> d_window;
    DevBuf<float4> d_tT;
    DevBuf<cf> d_cc;

    // window: the caller's kFftN floats or NULL for the periodic Hann window; a non-finite value is refused (before any
    // device call).  `what` names the block in the error text.
    gr4pm_status create(const float* window_in, hipStream_t s, const char* what)
    {
        std::vector<float> window(kFftN);
        if (window_in)
            std::copy(window_in, window_in + kFftN, window.begin());
        else
            hann(kFftN, window.data());
        window_power = 0.0;
        for (size_t i = 0; i < kFftN; ++i) {
            if (!std::isfinite(window[i])) {
                set_error("%s: window[%zu] is not finite", what, i);
                return GR4PM_ERR_INVALID;
            }
            window_power += static_cast<double>(window[i]) * static_cast<double>(window[i]);
        }
        GR4PM_TRY(require_device());
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
            max_waves = std::min(max_waves, static_cast<size_t>(prop.multiProcessorCount) * kW64Waves);
        std::vector<float4> tT(kW64TwFloat4);
        std::vector<cf> cc(64);
        build_w64_tables(
            [](int k) {
                const double ang = -2.0 * M_PI * k / kFftN;
                return mk(static_cast<float>(std::cos(ang)), static_cast<float>(std::sin(ang)));
            },
            tT.data(), cc.data());
        GR4PM_TRY(d_window.alloc(kFftN));
        GR4PM_TRY(d_tT.alloc(tT.size()));
        GR4PM_TRY(d_cc.alloc(cc.size()));
        GR4PM_TRY(d_window.upload(window.data(), kFftN, s));
        GR4PM_TRY(d_tT.upload(tT.data(), tT.size(), s));
        GR4PM_TRY(d_cc.upload(cc.data(), cc.size(), s));
        return GR4PM_OK;
    }
};

} // namespace
} // namespace gr4pm
