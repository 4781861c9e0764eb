// fft_ddc.hip -- K off-grid channels of one wideband stream from one shared transform: the fast-convolution (overlap-save)
// form of the Ddc for power-of-two decimations.  The project's own block (the reference is a one-channel modem).
// Definition (include/gr4pm_hip.h; the integer side is hostlogic/fft_ddc_plan.hpp's):
//     N = 2048, B = N / D, hop = N - V, segment s = the N items from a_s = s hop - V + D - 1 on, x = 0 before the start
//     X_s = FFT_N(x_s),  Z[u] = X_s[(c_k + u) mod N] G_k[u],  u in [-R B / 2, R B / 2)
//     Y[v] = sum_{u = v mod B} Z[u] (ascending u),  y'[n'] = sum_v Y[v] exp(+2 pi j v n' / B),  n' = V / D .. B - 1
//     out_k[s hop / D + n' - V / D] = exp(-2 pi j phi / 2^32) y'[n'],  phi = (w_k i - c_k 2^21 p) mod 2^32
//
// Two kernels, with the segments' whole spectra between them:
// k_fft_ddc_forward: the Spectrum's wave (spectrum.hip) without window and powers: one wave per run of consecutive
//   segments on the one-exchange transform of fft2048_w64.hpp, fed by load_half_segment(); register j of lane l holds
//   bin l + 64 j, and leaves as 32 rows of 64 consecutive bins to spec[segment][2048].
// k_fft_ddc_channel: one wave per (segment, channel).  Lane l takes the folded bins v = l, l + 64, ...: R products
//   X[(c + u) mod N] G[u] in ascending u, consecutive lanes on consecutive bins of the spectrum and of the table.  The
//   B-point inverse transform is log2 B radix-2 autosort (Stockham) stages between two LDS buffers, natural order in and
//   out, twiddles exp(+2 pi j m / 512) from a table made in double; then the kept items n' >= V / D take the rotator
//   (the Ddc's: double sincospi of the exact phase, rounded to float, four fmaf from zero) and leave as hop / D
//   consecutive frames of row k.
// A launch pair covers at most kChunk segments, so the spectra of a call of any length stay within one 64 MiB buffer
// that the next pair reuses in stream order.  No atomics, no scratch; every result is a function of (channel, frame,
// stream) only, whatever the cuts into calls.
// Built with FFT_FLAGS: the transforms, the products and the fold may contract to FMA.  The rotator is written in
// explicit fmaf (freq_xlate.hpp's cmac), so it is the Ddc's under either set of flags.
#include "spectrum_segment.hpp"
#include "freq_xlate.hpp"
#include "hostlogic/fft_ddc_plan.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

namespace {

namespace iq = gr4pm::iq;
using namespace gr4pm;
using gr4pm::hostlogic::fft_ddc_bin;
using gr4pm::hostlogic::fft_ddc_default_overlap;
using gr4pm::hostlogic::fft_ddc_phi;
using gr4pm::hostlogic::fft_ddc_plan;
using gr4pm::hostlogic::fft_ddc_pow2;
using gr4pm::hostlogic::fft_ddc_segment_index;
using gr4pm::hostlogic::fft_ddc_shape;
using gr4pm::hostlogic::fft_ddc_table_word;
using gr4pm::hostlogic::fft_ddc_validate;
using gr4pm::hostlogic::FftDdcPlan;
using gr4pm::hostlogic::FftDdcRefusal;
using gr4pm::hostlogic::FftDdcShape;
using gr4pm::hostlogic::kFftDdcMaxD;
using gr4pm::hostlogic::kFftDdcMaxK;
using gr4pm::hostlogic::kFftDdcMinD;
using gr4pm::hostlogic::kFftDdcMinHop;

constexpr size_t kN = kFftN;
constexpr size_t kChunk = 4096;  // segments of one launch pair: 64 MiB of spectra
constexpr int kTwiddles = 256;   // exp(+2 pi j m / 512), m < 256
constexpr int kMaxB = 512;

struct FwdArgs {
    const float2* hist; // the H carried items in front of in[0]
    const void* in;     // complex64, or items of the kernel's integer format
    size_t H;
    size_t seg0;        // the launch's first segment, counted from the call's
    const float4* tT;
    const cf* cc;
    cf* spec;           // [segments of the launch][2048]
    uint32_t n_seg;     // segments of the launch
    uint32_t run;       // per wave
    uint32_t hop;
    float scale;        // of an integer format's unpack
};

template <int F>
__global__ __launch_bounds__(kW64Threads, 2) void k_fft_ddc_forward(FwdArgs a)
{
    __shared__ float4 lds4[kW64LdsF4]; // twiddles | eight exchange buffers
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < kW64TwFloat4; i += kW64Threads) lds4[i] = a.tT[i];
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

    // segment `seg` of the launch begins at the virtual item (seg0 + seg) hop
    auto load_half = [&](cf* dst, uint64_t seg, int h) {
        load_half_segment<F>(dst, a.hist, a.H, a.in, a.scale, (a.seg0 + seg) * a.hop, lane, h);
    };

    cf X[32];
    load_half(X, first, 0);
    load_half(X, first, 1);
    for (uint32_t s = 0; s < count; ++s) {
        cf bq[32];
        dft32(X);
        w64_store(X, base);
        w64_mid_dev<1, true>(lane, row, ldsT, c, bq);
        // pass A's registers take the next segment, as in k_spectrum_w64: one half while pass B runs, one behind it
        const bool has_next = s + 1 < count;
        if (has_next) load_half(X, first + s + 1, 0);
        dft32(bq);
#pragma unroll
        for (int k = 0; k < 32; k += 4) w64_pin4(bq + k);
        if (has_next) load_half(X, first + s + 1, 1);
        cf* o = a.spec + (first + s) * kN + lane;
#pragma unroll
        for (int j = 0; j < 32; ++j) o[64 * j] = bq[j];
    }
}

struct ChanArgs {
    const float2* spec; // [segments of the launch][2048]
    const float2* G;    // [K][R B]: item t is u = t - R B / 2
    const float2* tw;   // [256]
    const uint32_t* w;  // [K] frequency words
    float2* out;
    size_t out_stride;
    size_t frame0;      // the launch's first frame of the call's rows
    uint64_t index0;    // absolute index of item 0 of the launch's first segment (its low 32 bits are all the phase needs)
    uint32_t n_seg;
    uint32_t D, logB, R;
    uint32_t first;     // V / D
    uint32_t hop;
};

// blockIdx.x: the segment of the launch, blockIdx.y: the channel; 64 threads
__global__ __launch_bounds__(64) void k_fft_ddc_channel(ChanArgs a)
{
    __shared__ float2 buf[2][kMaxB];
    __shared__ float2 tw[kTwiddles];
    const uint32_t lane = threadIdx.x;
    const uint32_t seg = blockIdx.x, k = blockIdx.y;
    const uint32_t B = 1u << a.logB, RB = a.R << a.logB;
    for (uint32_t m = lane; m < kTwiddles; m += 64) tw[m] = a.tw[m];

    const uint32_t wk = a.w[k], c = fft_ddc_bin(wk);
    const float2* __restrict__ X = a.spec + static_cast<size_t>(seg) * kN;
    const float2* __restrict__ G = a.G + static_cast<size_t>(k) * RB;
    const uint32_t bin0 = c + static_cast<uint32_t>(kN) - RB / 2; // bin of the table's item 0, before the wrap
    for (uint32_t v = lane; v < B; v += 64) {
        uint32_t t = (v + RB / 2) & (B - 1); // the table's first item of the folded bin v; the others are B apart
        float2 y = {0.0f, 0.0f};
        for (uint32_t r = 0; r < a.R; ++r, t += B) {
            const float2 x = X[(bin0 + t) & (kN - 1)], g = G[t];
            const float2 z = {x.x * g.x - x.y * g.y, x.x * g.y + x.y * g.x};
            if (r == 0)
                y = z;
            else
                y.x += z.x, y.y += z.y;
        }
        buf[0][v] = y;
    }
    __syncthreads();

    // stage of sub-transform length Ns: butterfly j takes items j and j + B / 2, position q = j mod Ns of its sub-transform,
    // and writes items (j - q) 2 + q and Ns later.  Natural order in, natural order out
    uint32_t src = 0;
    for (uint32_t ls = 0; ls < a.logB; ++ls) {
        const uint32_t Ns = 1u << ls;
        for (uint32_t j = lane; j < B / 2; j += 64) {
            const uint32_t q = j & (Ns - 1);
            const float2 t = tw[q << (8 - ls)]; // exp(+2 pi j q / (2 Ns))
            const float2 p = buf[src][j], b = buf[src][j + B / 2];
            const float2 e = {b.x * t.x - b.y * t.y, b.x * t.y + b.y * t.x};
            const uint32_t o = ((j - q) << 1) + q;
            buf[src ^ 1][o] = float2{p.x + e.x, p.y + e.y};
            buf[src ^ 1][o + Ns] = float2{p.x - e.x, p.y - e.y};
        }
        src ^= 1;
        __syncthreads();
    }

    const uint32_t frames = B - a.first;
    const uint32_t i0 = static_cast<uint32_t>(a.index0) + seg * a.hop;
    float2* __restrict__ o = a.out + static_cast<size_t>(k) * a.out_stride + a.frame0 + static_cast<size_t>(seg) * frames;
    for (uint32_t f = lane; f < frames; f += 64) {
        const uint32_t p = (a.first + f) * a.D;
        const uint32_t phi = fft_ddc_phi(wk, c, i0 + p, p);
        float2 y = {0.0f, 0.0f};
        cmac(y, mixer<-1>(phi, 1u), buf[src][a.first + f]);
        o[f] = y;
    }
}

// G_k[u] = (1 / N) sum_t h[t] exp(-2 pi j psi t / 2^32), psi = ((c_k + u) 2^21 - w_k) mod 2^32: the phase of every term an
// exact integer, the sum in double, each component rounded to float once
float2 response(const std::vector<float>& h, uint32_t w, uint32_t c, int32_t u)
{
    const uint32_t psi = fft_ddc_table_word(w, c, u);
    double re = 0.0, im = 0.0;
    for (size_t t = 0; t < h.size(); ++t) {
        double cs, sn;
        unit_phasor(0u - psi * static_cast<uint32_t>(t), cs, sn);
        re += static_cast<double>(h[t]) * cs;
        im += static_cast<double>(h[t]) * sn;
    }
    return float2{static_cast<float>(re / static_cast<double>(kN)), static_cast<float>(im / static_cast<double>(kN))};
}

gr4pm_status check_decimation(size_t D)
{
    if (!fft_ddc_pow2(D) || D < kFftDdcMinD || D > kFftDdcMaxD) {
        set_error("fft_ddc: the decimation must be a power of two in [%u, %u], not %zu", kFftDdcMinD, kFftDdcMaxD, D);
        return GR4PM_ERR_INVALID;
    }
    return GR4PM_OK;
}

} // namespace

struct gr4pm_fft_ddc {
    size_t K = 0, D = 0, R = 0, V = 0;
    uint64_t start_index = 0;
    uint64_t taken = 0; // samples since create or reset
    FftDdcShape shape = {};
    hipStream_t stream = nullptr;
    size_t max_waves = 2048; // of one forward launch: eight per compute unit, at most 2048
    std::vector<uint32_t> words;
    gr4pm::StreamTail tail; // keep = 0, frame = N: the virtual items of the incomplete segment
    gr4pm::DevBuf<float4> d_tT;
    gr4pm::DevBuf<cf> d_cc, d_spec;
    gr4pm::DevBuf<float2> d_G, d_tw;
    gr4pm::DevBuf<uint32_t> d_w;
};

// process() and process_iq(): format iq::kC64 for complex64 samples
static gr4pm_status process_any(gr4pm_fft_ddc* h, const void* in, int format, float scale, size_t n_in, gr4pm_c64* out,
                                size_t out_stride, size_t out_cap_frames, size_t* n_frames)
{
    if (!h || !n_frames) return GR4PM_ERR_INVALID;
    *n_frames = 0;
    if (n_in > (size_t(1) << 40)) {
        set_error("fft_ddc: %zu samples in one call, at most 2^40", n_in);
        return GR4PM_ERR_OVERFLOW;
    }
    if (n_in == 0) return GR4PM_OK;
    if (!in) {
        set_error("fft_ddc: no input array");
        return GR4PM_ERR_INVALID;
    }
    const FftDdcPlan p = fft_ddc_plan(h->shape, h->taken, n_in);
    if (p.frames > out_cap_frames) {
        set_error("fft_ddc: %zu frames, room for %zu", p.frames, out_cap_frames);
        return GR4PM_ERR_OVERFLOW;
    }
    if (p.frames && (!out || (h->K > 1 && out_stride < p.frames))) {
        set_error("fft_ddc: no output array, or a row stride of %zu items for %zu frames", out_stride, p.frames);
        return GR4PM_ERR_INVALID;
    }
    // the samples in front of the virtual stream (V = 0 only) belong to no frame
    const size_t item = format == iq::kC64 ? sizeof(float2) : iq::item_bytes(format);
    const void* x = static_cast<const char*>(in) + p.drop * item;
    const StreamTail::Plan t = {h->tail.d_hist[h->tail.cur].p, h->tail.d_hist[1 - h->tail.cur].p, p.tail, p.n_segments,
                                p.tail_new, p.tail_new};
    FwdArgs a = {};
    a.hist = t.hist, a.in = x, a.H = p.tail;
    a.tT = h->d_tT.p, a.cc = h->d_cc.p, a.spec = h->d_spec.p;
    a.hop = h->shape.hop, a.scale = scale;
    ChanArgs b = {};
    b.spec = reinterpret_cast<const float2*>(h->d_spec.p), b.G = h->d_G.p, b.tw = h->d_tw.p, b.w = h->d_w.p;
    b.out = reinterpret_cast<float2*>(out), b.out_stride = out_stride;
    b.D = static_cast<uint32_t>(h->D), b.R = static_cast<uint32_t>(h->R);
    b.logB = static_cast<uint32_t>(__builtin_ctzll(kN / h->D));
    b.first = h->shape.first, b.hop = h->shape.hop;
    iq::with_format(format, [&](auto f) {
        for (size_t done = 0; done < p.n_segments;) {
            const size_t segs = std::min(p.n_segments - done, kChunk);
            const size_t run = (segs + h->max_waves - 1) / h->max_waves;
            const size_t waves = (segs + run - 1) / run;
            a.seg0 = done, a.n_seg = static_cast<uint32_t>(segs), a.run = static_cast<uint32_t>(run);
            hipLaunchKernelGGL(k_fft_ddc_forward<decltype(f)::value>, dim3(static_cast<unsigned>((waves + kW64Waves - 1) / kW64Waves)),
                               dim3(kW64Threads), 0, h->stream, a);
            b.n_seg = a.n_seg;
            b.frame0 = done * h->shape.frames;
            b.index0 = fft_ddc_segment_index(h->shape, h->start_index, p.segments_before + done);
            hipLaunchKernelGGL(k_fft_ddc_channel, dim3(static_cast<unsigned>(segs), static_cast<unsigned>(h->K)), dim3(64), 0,
                               h->stream, b);
            done += segs;
        }
        h->tail.launch_history<decltype(f)::value>(t, x, 0, p.n_used, scale, h->stream);
    });
    GR4PM_HIP_TRY(hipGetLastError());
    h->tail.commit(t);
    h->taken += n_in;
    *n_frames = p.frames;
    return GR4PM_OK;
}

extern "C" {

gr4pm_status gr4pm_fft_ddc_taps(size_t decimation, size_t taps_per_phase, float* out)
try {
    if (!out) return GR4PM_ERR_INVALID;
    GR4PM_TRY(check_decimation(decimation));
    return gr4pm_ddc_taps(decimation, taps_per_phase, 0.25, 0.75, out);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_ddc_create(const gr4pm_fft_ddc_params* p, gr4pm_fft_ddc** out)
try {
    if (!p || !out) return GR4PM_ERR_INVALID;
    *out = nullptr;
    const size_t K = p->n_channels, D = p->decimation, R = p->images;
    std::vector<uint32_t> words;
    GR4PM_TRY(frequency_words("fft_ddc", p->frequencies, K, kFftDdcMaxK, words));
    GR4PM_TRY(check_decimation(D));
    if (!fft_ddc_pow2(R) || R > D) {
        set_error("fft_ddc: images must be a power of two in [1, %zu], not %zu", D, R);
        return GR4PM_ERR_INVALID;
    }
    GR4PM_TRY(prototype_length("fft_ddc", p->taps, p->n_taps, kN));
    std::vector<float> taps;
    if (p->taps) {
        taps.assign(p->taps, p->taps + p->n_taps);
    } else {
        if (p->taps_per_phase < 1 || p->taps_per_phase * D > kN) {
            set_error("fft_ddc: %zu taps per phase at a decimation of %zu: the prototype has 1 .. %zu taps", p->taps_per_phase, D, kN);
            return GR4PM_ERR_INVALID;
        }
        taps.resize(p->taps_per_phase * D);
        GR4PM_TRY(gr4pm_ddc_taps(D, p->taps_per_phase, 0.25, 0.75, taps.data()));
    }
    const size_t L = taps.size();
    for (size_t t = 0; t < L; ++t)
        if (!std::isfinite(taps[t])) {
            set_error("fft_ddc: taps[%zu] is not finite", t);
            return GR4PM_ERR_INVALID;
        }
    const size_t V = p->overlap < 0 ? fft_ddc_default_overlap(L) : static_cast<size_t>(p->overlap);
    switch (fft_ddc_validate(K, D, R, L, V)) {
    case FftDdcRefusal::none: break;
    case FftDdcRefusal::overlap_multiple:
        set_error("fft_ddc: the overlap %zu is no multiple of the decimation %zu", V, D);
        return GR4PM_ERR_INVALID;
    case FftDdcRefusal::overlap_low:
        set_error("fft_ddc: the overlap %zu is below the %zu taps' reach of %zu samples", V, L, L - 1);
        return GR4PM_ERR_INVALID;
    case FftDdcRefusal::overlap_high:
        set_error("fft_ddc: the overlap %zu leaves a hop below %u: at most %zu", V, kFftDdcMinHop, kN - kFftDdcMinHop);
        return GR4PM_ERR_INVALID;
    default: set_error("fft_ddc: invalid sizes"); return GR4PM_ERR_INVALID;
    }
    GR4PM_TRY(require_device());
    std::unique_ptr<gr4pm_fft_ddc> h(new (std::nothrow) gr4pm_fft_ddc);
    if (!h) return GR4PM_ERR_NOMEM;
    h->K = K, h->D = D, h->R = R, h->V = V;
    h->start_index = p->start_index;
    h->shape = fft_ddc_shape(static_cast<uint32_t>(D), static_cast<uint32_t>(V));
    h->stream = static_cast<hipStream_t>(p->stream);
    h->words = std::move(words);
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
        h->max_waves = std::min(h->max_waves, static_cast<size_t>(prop.multiProcessorCount) * kW64Waves);

    std::vector<float4> tT(kW64TwFloat4);
    std::vector<cf> cc(64);
    build_w64_tables(
        [](int k) {
            const double ang = -2.0 * M_PI * k / kFftN;
            return mk(static_cast<float>(std::cos(ang)), static_cast<float>(std::sin(ang)));
        },
        tT.data(), cc.data());
    std::vector<float2> tw(kTwiddles);
    for (int m = 0; m < kTwiddles; ++m) {
        double cs, sn;
        unit_phasor(static_cast<uint32_t>(m) << 23, cs, sn); // m / 512 of a turn
        tw[m] = float2{static_cast<float>(cs), static_cast<float>(sn)};
    }
    const size_t B = kN / D, RB = R * B;
    std::vector<float2> G(K * RB);
    for (size_t k = 0; k < K; ++k) {
        const uint32_t w = h->words[k], c = fft_ddc_bin(w);
        for (size_t t = 0; t < RB; ++t) G[k * RB + t] = response(taps, w, c, static_cast<int32_t>(t) - static_cast<int32_t>(RB / 2));
    }
    GR4PM_TRY(h->d_tT.alloc(tT.size()));
    GR4PM_TRY(h->d_cc.alloc(cc.size()));
    GR4PM_TRY(h->d_tw.alloc(tw.size()));
    GR4PM_TRY(h->d_G.alloc(G.size()));
    GR4PM_TRY(h->d_w.alloc(K));
    GR4PM_TRY(h->d_spec.alloc(kChunk * kN));
    GR4PM_TRY(h->d_tT.upload(tT.data(), tT.size(), h->stream));
    GR4PM_TRY(h->d_cc.upload(cc.data(), cc.size(), h->stream));
    GR4PM_TRY(h->d_tw.upload(tw.data(), tw.size(), h->stream));
    GR4PM_TRY(h->d_G.upload(G.data(), G.size(), h->stream));
    GR4PM_TRY(h->d_w.upload(h->words.data(), K, h->stream));
    GR4PM_TRY(h->tail.alloc(0, kN, 1, h->stream));
    return finish_create(h, out, "fft_ddc");
}
GR4PM_ABI_CATCH

void gr4pm_fft_ddc_destroy(gr4pm_fft_ddc* h)
try {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    delete h;
}
GR4PM_ABI_CATCH_VOID

gr4pm_status gr4pm_fft_ddc_reset(gr4pm_fft_ddc* h)
try {
    if (!h) return GR4PM_ERR_INVALID;
    GR4PM_TRY(h->tail.reset(h->stream));
    h->taken = 0;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_ddc_frames_for(const gr4pm_fft_ddc* h, size_t n_in, size_t* n_frames)
try {
    if (!h || !n_frames) return GR4PM_ERR_INVALID;
    *n_frames = 0;
    if (n_in > (size_t(1) << 40)) {
        set_error("fft_ddc: %zu samples in one call, at most 2^40", n_in);
        return GR4PM_ERR_OVERFLOW;
    }
    *n_frames = fft_ddc_plan(h->shape, h->taken, n_in).frames;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_ddc_frequencies(const gr4pm_fft_ddc* h, double* out)
try {
    if (!h || !out) return GR4PM_ERR_INVALID;
    for (size_t k = 0; k < h->K; ++k) out[k] = folded_frequency(h->words[k]);
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_ddc_sizes(const gr4pm_fft_ddc* h, size_t* overlap, size_t* hop)
try {
    if (!h || !overlap || !hop) return GR4PM_ERR_INVALID;
    *overlap = h->V;
    *hop = h->shape.hop;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_ddc_process(gr4pm_fft_ddc* h, const gr4pm_c64* in, size_t n_in, gr4pm_c64* out, size_t out_stride,
                                   size_t out_cap_frames, size_t* n_frames)
try {
    return process_any(h, in, iq::kC64, 0.0f, n_in, out, out_stride, out_cap_frames, n_frames);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_ddc_process_iq(gr4pm_fft_ddc* h, const void* in, int format, float scale, size_t n_in, gr4pm_c64* out,
                                      size_t out_stride, size_t out_cap_frames, size_t* n_frames)
try {
    if (n_frames) *n_frames = 0;
    if (!iq::valid(format)) {
        set_error("fft_ddc: format %d is none of GR4PM_IQ_SC16 / SC8 / CU8", format);
        return GR4PM_ERR_INVALID;
    }
    return process_any(h, in, format, scale == 0.0f ? iq::default_scale(format) : scale, n_in, out, out_stride, out_cap_frames,
                       n_frames);
}
GR4PM_ABI_CATCH

} // extern "C"
