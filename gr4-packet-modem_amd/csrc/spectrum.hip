// spectrum.hip -- Welch power spectral density of one wideband stream, and the host-only carrier finder made from it.
// The project's own block (the reference has none).  Definition (include/gr4pm_hip.h):
//     segment s = x[s hop .. s hop + N), N = 2048, 1 <= hop <= N, no zero prehistory
//     X_s = FFT_N(w . x_s),  acc[k] = sum_s |X_s[k]|^2,  max[k] = max_s |X_s[k]|^2
//
// k_spectrum_w64: one wave per run of consecutive segments, on the one-exchange wave transform of fft2048_w64.hpp, whose
//   input and output distributions coincide: register j of lane l holds index l + 64 j.  So a wave loads a segment in
//   rows of 64 consecutive samples, multiplies by the window (w[lane + 64 j]: rows of 64 floats, read from LDS where
//   they are used), transforms, and forms |X|^2 in the registers where the outputs land -- where its 32 sums and 32
//   maxima line up with them.  Half of the next segment is requested when the exchange has freed pass A's registers
//   and arrives while pass B runs, the other half when pass B is complete.  A sample comes through iq::vsample() when
//   the segment begins in the carried tail (tail ++ input is one virtual stream), straight from the input otherwise;
//   an integer format converts right there.
//   Eight waves of 16.5 KiB exchange buffers per workgroup, the layout of k_correlate_w64, not the twelve of 8.5 KiB of
//   k_correlate_w64_one: sums and maxima are 64 registers that live for the whole run, beside 64 of a transform, its
//   temporaries and the samples in flight, which three waves per SIMD (168 registers) cannot hold.  The window does not
//   live in registers either: with it there (96 registers for the run) the kernel fits 256 registers only without any
//   load in flight during the arithmetic (250, and 112 spilled with the prefetch); in LDS it is 8 KiB beside the 151.5,
//   32 conflict-free ds_read_b32 a segment, and the kernel has 248 registers and no scratch.
//   A wave sums at most kFloatRun = 64 segments in float32, then writes its sums and maxima as rows (lane + 64 j:
//   coalesced) to partials[wave][2][2048].
// k_spectrum_reduce: per bin, the partial sums in wave order in float64 into the handle's acc[2048], the maxima into
//   max[2048].  No floating-point atomic anywhere: the same calls give the same bits.
// The carried tail is stream_tail.hpp's two buffers and its kernel with keep = 0, frame = N: the tail IS the incomplete
// segment; what a call completes and leaves behind is hostlogic/spectrum_plan.hpp's, since segments begin at multiples of
// hop but end N later, which is no multiple of hop in general.
// Built with FFT_FLAGS: the transform may contract to FMA.  iq_format.hpp's unpack is one product (cu8: a difference, then
// one product), in which there is nothing to contract, so it is gr4pm_iq_unpack's expression bit for bit here too.
#include "spectrum_segment.hpp"
#include "hostlogic/carrier_find.hpp"
#include "hostlogic/spectrum_plan.hpp"

#include <algorithm>
#include <cmath>

namespace {

namespace iq = gr4pm::iq;
using namespace gr4pm;
using gr4pm::hostlogic::spectrum_plan;
using gr4pm::hostlogic::SpectrumPlan;

constexpr uint32_t kFloatRun = 64; // segments a wave sums in float32: the error bound of DESIGN.md section 20 rests on it
constexpr size_t kN = kFftN;

struct SpecArgs {
    const float2* hist; // the H carried samples in front of in[0]
    const void* in;     // complex64, or items of the kernel's integer format
    size_t H;
    size_t seg0;        // the launch's first segment, counted from the virtual stream's item 0
    const float* window;
    const float4* tT;
    const cf* cc;
    float* part;        // [waves][2][2048]
    uint32_t n_seg;     // segments of the launch
    uint32_t run;       // per wave, <= kFloatRun
    uint32_t hop;
    float scale;        // of an integer format's unpack
};

template <int F>
__global__ __launch_bounds__(kW64Threads, 2) void k_spectrum_w64(SpecArgs a)
{
    __shared__ float4 lds4[kW64LdsF4 + kFftN / 4]; // twiddles | eight exchange buffers | the window
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < kW64TwFloat4; i += kW64Threads) lds4[i] = a.tT[i];
    for (int i = tid; i < kFftN / 4; i += kW64Threads) lds4[kW64LdsF4 + i] = reinterpret_cast<const float4*>(a.window)[i];
    __syncthreads(); // the only workgroup-wide synchronisation of the kernel
    float4* xb4 = lds4 + kW64TwFloat4 + wave * kW64BufF4;
    const uint32_t base = __builtin_amdgcn_readfirstlane(
        static_cast<uint32_t>(reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) char*)xb4)));
    const float4* row = xb4 + (lane & 31) * (kW64Row / 4);
    const float4* ldsT = lds4;
    const cf c = a.cc[lane];

    const uint32_t w = blockIdx.x * kW64Waves + wave;
    const uint64_t first = static_cast<uint64_t>(w) * a.run;
    if (first >= a.n_seg) return;
    const uint32_t count = a.n_seg - first < a.run ? static_cast<uint32_t>(a.n_seg - first) : a.run;

    const float* wl = reinterpret_cast<const float*>(lds4 + kW64LdsF4) + lane; // w[lane + 64 j]: a row of 64 per read
    float sum[32], mx[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        sum[j] = 0.0f;
        mx[j] = 0.0f;
    }
    // segment `seg` of the launch begins at the virtual item (seg0 + seg) hop
    auto load_half = [&](cf* dst, uint64_t seg, int h) {
        load_half_segment<F>(dst, a.hist, a.H, a.in, a.scale, (a.seg0 + seg) * a.hop, lane, h);
    };

    cf X[32];
    load_half(X, first, 0);
    load_half(X, first, 1);
    for (uint32_t s = 0; s < count; ++s) {
#pragma unroll
        for (int j = 0; j < 32; ++j) X[j] = X[j] * dup_x(mk(wl[64 * j], 0.0f));
        cf bq[32];
        dft32(X);
        w64_store(X, base);
        w64_mid_dev<1, true>(lane, row, ldsT, c, bq);
        // pass A's registers are dead: they take the next segment -- one half now (it arrives while pass B runs; both
        // halves in flight beside pass B's temporaries and the 96 registers of the run would spill), the other when pass B
        // is complete (the pin: hipcc otherwise hoists those loads above the arithmetic)
        const bool has_next = s + 1 < count;
        if (has_next) load_half(X, first + s + 1, 0);
        dft32(bq);
#pragma unroll
        for (int k = 0; k < 32; k += 4) w64_pin4(bq + k);
        if (has_next) load_half(X, first + s + 1, 1);
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const float p = fmaf(bq[j].y, bq[j].y, bq[j].x * bq[j].x);
            sum[j] += p;
            mx[j] = __builtin_fmaxf(mx[j], p);
        }
    }
    float* ps = a.part + static_cast<size_t>(w) * (2 * kFftN) + lane;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        ps[64 * j] = sum[j];
        ps[kFftN + 64 * j] = mx[j];
    }
}

// 2048 threads, one per bin; the partials of `waves` waves in wave order
__global__ __launch_bounds__(64) void k_spectrum_reduce(const float* __restrict__ part, uint32_t waves, double* __restrict__ acc,
                                                        float* __restrict__ mx)
{
    const uint32_t k = blockIdx.x * 64 + threadIdx.x;
    double a = acc[k];
    float m = mx[k];
    const float* p = part + k;
    uint32_t w = 0;
    for (; w + 8 <= waves; w += 8) { // eight waves' loads in flight, added in order
        float s[8], q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            s[u] = p[static_cast<size_t>(w + u) * (2 * kFftN)];
            q[u] = p[static_cast<size_t>(w + u) * (2 * kFftN) + kFftN];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            a += static_cast<double>(s[u]);
            m = fmaxf(m, q[u]);
        }
    }
    for (; w < waves; ++w) {
        a += static_cast<double>(p[static_cast<size_t>(w) * (2 * kFftN)]);
        m = fmaxf(m, p[static_cast<size_t>(w) * (2 * kFftN) + kFftN]);
    }
    acc[k] = a;
    mx[k] = m;
}

} // namespace

struct gr4pm_spectrum {
    size_t hop = 0;
    uint64_t taken = 0;    // T: samples since create or reset
    uint64_t segments = 0;
    hipStream_t stream = nullptr;
    gr4pm::SegmentTransform tf; // the window and its power, the transform's tables, the waves of one launch
    gr4pm::StreamTail tail;     // keep = 0, frame = N: the samples of the incomplete segment
    gr4pm::DevBuf<float> d_part, d_max;
    gr4pm::DevBuf<double> d_acc;
};

// process() and process_iq(): format iq::kC64 for complex64 samples
static gr4pm_status process_any(gr4pm_spectrum* h, const void* x, int format, float scale, size_t n)
{
    if (!h) return GR4PM_ERR_INVALID;
    if (n > (size_t(1) << 40)) {
        set_error("spectrum: %zu samples in one call, at most 2^40", n);
        return GR4PM_ERR_OVERFLOW;
    }
    if (n == 0) return GR4PM_OK;
    if (!x) {
        set_error("spectrum: no input array");
        return GR4PM_ERR_INVALID;
    }
    const SpectrumPlan p = spectrum_plan(h->taken, n, kN, h->hop);
    const StreamTail::Plan t = {h->tail.d_hist[h->tail.cur].p, h->tail.d_hist[1 - h->tail.cur].p, p.tail, p.n_segments,
                                p.tail_new, p.tail_new};
    SpecArgs a = {};
    a.hist = t.hist, a.in = x, a.H = p.tail;
    a.window = h->tf.d_window.p, a.tT = h->tf.d_tT.p, a.cc = h->tf.d_cc.p, a.part = h->d_part.p;
    a.hop = static_cast<uint32_t>(h->hop), a.scale = scale;
    iq::with_format(format, [&](auto f) {
        for (size_t done = 0; done < p.n_segments;) {
            const size_t left = p.n_segments - done;
            const size_t run = hostlogic::spectrum_run(left, h->tf.max_waves, kFloatRun);
            const size_t waves = std::min(h->tf.max_waves, (left + run - 1) / run);
            const size_t segs = std::min(left, waves * run);
            a.seg0 = done, a.n_seg = static_cast<uint32_t>(segs), a.run = static_cast<uint32_t>(run);
            hipLaunchKernelGGL(k_spectrum_w64<decltype(f)::value>, dim3(static_cast<unsigned>((waves + kW64Waves - 1) / kW64Waves)),
                               dim3(kW64Threads), 0, h->stream, a);
            hipLaunchKernelGGL(k_spectrum_reduce, dim3(kFftN / 64), dim3(64), 0, h->stream, h->d_part.p,
                               static_cast<uint32_t>(waves), h->d_acc.p, h->d_max.p);
            done += segs;
        }
        h->tail.launch_history<decltype(f)::value>(t, x, 0, n, scale, h->stream);
    });
    GR4PM_HIP_TRY(hipGetLastError());
    h->tail.commit(t);
    h->taken += n;
    h->segments += p.n_segments;
    return GR4PM_OK;
}

extern "C" {

gr4pm_status gr4pm_spectrum_window(uint32_t n, float* out)
try {
    if (!out && n) return GR4PM_ERR_INVALID;
    hann(n, out);
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

uint32_t gr4pm_spectrum_float_run(void)
try {
    return kFloatRun;
}
GR4PM_ABI_CATCH_RET(0)

gr4pm_status gr4pm_spectrum_create(const gr4pm_spectrum_params* p, gr4pm_spectrum** out)
try {
    if (!p || !out) return GR4PM_ERR_INVALID;
    *out = nullptr;
    if (p->fft_size != kN) {
        set_error("spectrum: fft_size %u, only 2048 exists", p->fft_size);
        return GR4PM_ERR_INVALID;
    }
    if (p->hop == 0 || p->hop > kN) {
        set_error("spectrum: hop %u, need 1 .. %zu", p->hop, kN);
        return GR4PM_ERR_INVALID;
    }
    std::unique_ptr<gr4pm_spectrum> h(new (std::nothrow) gr4pm_spectrum);
    if (!h) return GR4PM_ERR_NOMEM;
    h->hop = p->hop;
    h->stream = static_cast<hipStream_t>(p->stream);
    GR4PM_TRY(h->tf.create(p->window, h->stream, "spectrum"));
    GR4PM_TRY(h->d_part.alloc(h->tf.max_waves * 2 * kN));
    GR4PM_TRY(h->d_acc.alloc(kN));
    GR4PM_TRY(h->d_max.alloc(kN));
    GR4PM_TRY(h->d_acc.zero(h->stream));
    GR4PM_TRY(h->d_max.zero(h->stream));
    GR4PM_TRY(h->tail.alloc(0, kN, 1, h->stream));
    return finish_create(h, out, "spectrum");
}
GR4PM_ABI_CATCH

void gr4pm_spectrum_destroy(gr4pm_spectrum* h)
try {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    delete h;
}
GR4PM_ABI_CATCH_VOID

gr4pm_status gr4pm_spectrum_reset(gr4pm_spectrum* h)
try {
    if (!h) return GR4PM_ERR_INVALID;
    GR4PM_TRY(h->tail.reset(h->stream));
    GR4PM_TRY(h->d_acc.zero(h->stream));
    GR4PM_TRY(h->d_max.zero(h->stream));
    h->taken = 0;
    h->segments = 0;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_spectrum_process(gr4pm_spectrum* h, const void* x, size_t n)
try {
    return process_any(h, x, iq::kC64, 0.0f, n);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_spectrum_process_iq(gr4pm_spectrum* h, const void* x, int format, float scale, size_t n)
try {
    if (!iq::valid(format)) {
        set_error("spectrum: format %d is none of GR4PM_IQ_SC16 / SC8 / CU8", format);
        return GR4PM_ERR_INVALID;
    }
    return process_any(h, x, format, scale == 0.0f ? iq::default_scale(format) : scale, n);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_spectrum_read(gr4pm_spectrum* h, double* mean, float* max_hold, uint64_t* segments)
try {
    if (!h) return GR4PM_ERR_INVALID;
    std::vector<double> acc(kN);
    std::vector<float> mx(kN);
    GR4PM_HIP_TRY(hipMemcpyAsync(acc.data(), h->d_acc.p, kN * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    GR4PM_HIP_TRY(hipMemcpyAsync(mx.data(), h->d_max.p, kN * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    GR4PM_HIP_TRY(hipStreamSynchronize(h->stream));
    if (segments) *segments = h->segments;
    const double per_mean = static_cast<double>(h->segments) * h->tf.window_power;
    for (size_t k = 0; k < kN; ++k) {
        if (mean) mean[k] = h->segments ? acc[k] / per_mean : 0.0;
        if (max_hold) max_hold[k] = h->segments ? static_cast<float>(static_cast<double>(mx[k]) / h->tf.window_power) : 0.0f;
    }
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_find_carriers(const double* psd, size_t n, const gr4pm_carrier_params* p, gr4pm_carrier* out, size_t cap,
                                 size_t* count)
try {
    if (count) *count = 0;
    if (!psd || !n || !p || !count || (cap && !out)) return GR4PM_ERR_INVALID;
    if (!(p->threshold_db > 0.0)) {
        set_error("find_carriers: threshold_db must be positive");
        return GR4PM_ERR_INVALID;
    }
    *count = hostlogic::find_carriers(psd, n, p->threshold_db, p->max_gap_bins, p->min_width_bins, out, cap);
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

} // extern "C"
