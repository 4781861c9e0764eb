// stream_tail.hpp -- what the front-end blocks that take one stream in calls of any length share (channelizer.hip,
// ddc.hip, duc.hip): the dispatch on the input's format, the read of a sample of "history, then this call's input",
// the kernel and the host-side state that carry a stream's tail from call to call, and three small loops of create().
// The tail: per row, the `keep` items a call's first frame reaches back to, then the items of the incomplete frame
// (`carried`, below `frame`).  It lives in one of two device buffers; a call reads one and k_stream_history writes the
// other, so a call shorter than the tail can take most of the new tail from the old one.
#pragma once
#include "iq_format.hpp"

#include <type_traits>
#include <vector>

namespace gr4pm {
namespace iq {

// fn(std::integral_constant<int, F>) for the runtime format: an integer format, anything else is complex64 (kC64)
// (iq_format.hip's converters keep their own three-way chains: they have no complex64 form to instantiate)
template <typename Fn>
void with_format(int format, Fn&& fn)
{
    switch (format) {
    case GR4PM_IQ_SC16: fn(std::integral_constant<int, GR4PM_IQ_SC16>{}); break;
    case GR4PM_IQ_SC8: fn(std::integral_constant<int, GR4PM_IQ_SC8>{}); break;
    case GR4PM_IQ_CU8: fn(std::integral_constant<int, GR4PM_IQ_CU8>{}); break;
    default: fn(std::integral_constant<int, kC64>{}); break;
    }
}

// sample v of the virtual stream hist[0 .. H) ++ in[0 ..): an integer item converts here, with unpack_item().  The
// values come by reference so that a kernel's argument members are read where the expression uses them, as they were
// when every kernel had this function to itself: the hot kernels compile to the instructions they had then.
template <int F>
__device__ __forceinline__ float2 vsample(const float2* const& hist, const size_t& H, const void* const& in,
                                          const float& scale, size_t v)
{
    if constexpr (F == kC64)
        return v < H ? hist[v] : static_cast<const float2*>(in)[v - H];
    else
        return v < H ? hist[v] : unpack_item<F>(load_item<F>(in, v - H), scale);
}

} // namespace iq

namespace { // internal linkage: the library has one code object per unit, each with its own copy

// blockIdx.y: the row.  Its virtual stream is hist[row][0 .. H) ++ in[row in_stride ..][0 .. n_in); the last H_new
// items of it go to hist_new[row][0 .. H_new)
template <int F>
__global__ __launch_bounds__(256) void k_stream_history(const float2* hist, size_t H, const void* in, size_t in_stride,
                                                        size_t n_in, float scale, float2* hist_new, size_t H_new)
{
    const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x, row = blockIdx.y;
    if (i >= H_new) return;
    const void* in_row;
    if constexpr (F == iq::kC64)
        in_row = static_cast<const float2*>(in) + row * in_stride;
    else
        in_row = static_cast<const unsigned char*>(in) + row * in_stride * iq::Fmt<F>::item_bytes;
    hist_new[row * H_new + i] = iq::vsample<F>(hist + row * H, H, in_row, scale, H + n_in - H_new + i);
}

} // namespace

// the host side of a handle's tail
struct StreamTail {
    size_t keep = 0, frame = 1, rows = 1;
    size_t carried = 0; // items of the incomplete frame, < frame
    int cur = 0;        // which buffer holds the tail
    DevBuf<float2> d_hist[2];

    // one call: the tail in front of it, what it completes and what it leaves behind
    struct Plan {
        const float2* hist;
        float2* hist_new;
        size_t H, n_frames, carried_new, H_new;
    };

    gr4pm_status alloc(size_t keep_, size_t frame_, size_t rows_, hipStream_t s)
    {
        keep = keep_, frame = frame_, rows = rows_;
        for (auto& d : d_hist) {
            GR4PM_TRY(d.alloc(rows * (keep + frame - 1)));
            GR4PM_TRY(d.zero(s));
        }
        return GR4PM_OK;
    }
    // the fresh stream: zero history, nothing carried
    gr4pm_status reset(hipStream_t s)
    {
        GR4PM_TRY(d_hist[cur].zero(s));
        carried = 0;
        return GR4PM_OK;
    }
    size_t frames(size_t n_in) const { return (carried + n_in) / frame; }
    Plan plan(size_t n_in) const
    {
        const size_t carried_new = (carried + n_in) % frame;
        return Plan{d_hist[cur].p, d_hist[1 - cur].p, keep + carried, frames(n_in), carried_new, keep + carried_new};
    }
    // after the block's own kernel, which reads p.hist: the new tail into the other buffer (no tail, no launch)
    template <int F>
    void launch_history(const Plan& p, const void* in, size_t in_stride, size_t n_in, float scale, hipStream_t s) const
    {
        if (p.H_new)
            hipLaunchKernelGGL(k_stream_history<F>, dim3(static_cast<unsigned>((p.H_new + 255) / 256), static_cast<unsigned>(rows)),
                               dim3(256), 0, s, p.hist, p.H, in, in_stride, n_in, scale, p.hist_new, p.H_new);
    }
    // once the launches succeeded.  The buffers swap only when the history kernel ran
    void commit(const Plan& p)
    {
        if (p.H_new) cur = 1 - cur;
        carried = p.carried_new;
    }
};

// a design made in double, each tap rounded to float once
inline void round_taps(const std::vector<double>& h, float* out)
{
    for (size_t t = 0; t < h.size(); ++t) out[t] = static_cast<float>(h[t]);
}

// a create()'s prototype: the caller's n taps, or what design(std::vector<double>&) makes
template <typename Design>
gr4pm_status taps_or_design(const float* taps, size_t n, Design&& design, std::vector<float>& out)
{
    if (taps) {
        out.assign(taps, taps + n);
        return GR4PM_OK;
    }
    std::vector<double> h;
    GR4PM_TRY(design(h));
    out.resize(h.size());
    round_taps(h, out.data());
    return GR4PM_OK;
}

} // namespace gr4pm
