// fft_filter.hip -- the FftFilter block: any complex FIR of up to 1985 taps on one wideband stream by fast convolution
// (overlap-save), and the host-only band-stop / band-pass designer.  The project's own block (the reference has none).
// Definition (include/gr4pm_hip.h):
//     N = 2048, taps h[0 .. L - 1], overlap V with L - 1 <= V <= N - 64, hop = N - V, x[i] = 0 for i < 0
//     segment s = the N items from s hop - V;  X_s = FFT_N(x_s);  G[k] = (1 / N) sum_t h[t] exp(-2 pi j k t / N)
//     y_s = N IFFT_N(X_s G);  out[s hop + p - V] = y_s[p] for p = V .. N - 1:  out[n] = sum_t h[t] x[n - t]
//
// k_fft_filter<F>: the correlator's chain with samples stored where it stores powers.  One wave per run of consecutive
//   segments on the one-exchange wave transform of fft2048_w64.hpp, whose input and output distributions coincide
//   (register j of lane l holds index l + 64 j): a wave loads a segment in rows of 64 consecutive samples
//   (load_half_segment<F>: through the carried tail where the segment begins in it, an integer format converted right
//   there), transforms, multiplies every bin by its entry of the table, transforms again and stores the rows p >= V.
//   The inverse is the forward transform on swapped components: N IFFT(Z) = swap(FFT(swap(Z))).  The table holds
//   W[k] = (Im G[k], Re G[k]), so that one packed multiply and one packed multiply-add make swap(X G) = conj(X) W from X,
//   and the store swaps back, as k_fft_duc_inverse's does.  The table is laid out as the lanes read it: float4 u of lane l
//   is (W[l + 128 u], W[l + 128 u + 64]), registers 2 u and 2 u + 1, so a wave's sixteen 16-byte loads are 1 KiB each.
//   The next segment's samples are requested when the second transform's exchange has freed the registers of its first
//   pass: one half in front of the last pass, the other behind it, as in k_spectrum_w64 and k_fft_duc_inverse.
//   Eight waves and the LDS image of k_fft_duc_inverse (twiddles | eight private exchange buffers, 151 552 B), one barrier.
// The carried tail is stream_tail.hpp's with keep = V, frame = hop, one row; the arithmetic of a call, of flush() and every
// refusal's condition are hostlogic/fft_filter_plan.hpp's, the designer is hostlogic/band_filter_design.hpp.
// Built with FFT_FLAGS: the transforms may contract to FMA; every segment goes through the same instructions whatever call
// brings it, so any cutting of the stream gives the same bits.
#include "spectrum_segment.hpp"
#include "hostlogic/band_filter_design.hpp"
#include "hostlogic/fft_filter_plan.hpp"

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

namespace {

namespace iq = gr4pm::iq;
using namespace gr4pm;
using hostlogic::band_filter_design;
using hostlogic::fft_filter_call_fits;
using hostlogic::fft_filter_check_new_taps;
using hostlogic::fft_filter_check_sizes;
using hostlogic::fft_filter_default_overlap;
using hostlogic::fft_filter_first_bad_tap;
using hostlogic::fft_filter_flush;
using hostlogic::fft_filter_plan;
using hostlogic::fft_filter_refuses;
using hostlogic::fft_filter_shape;
using hostlogic::FftFilterFlush;
using hostlogic::FftFilterPlan;
using hostlogic::FftFilterShape;
using hostlogic::FftFilterSizes;
using hostlogic::kFftFilterMaxOverlap;
using hostlogic::kFftFilterMaxTaps;
using hostlogic::kFftFilterN;

constexpr size_t kN = kFftN;
static_assert(kN == kFftFilterN, "the plan's N is the transform's");
constexpr size_t kChunk = size_t(1) << 20; // segments of one launch at most: its counters are 32 bits wide

struct FilterArgs {
    const float2* hist; // the H carried items in front of in[0]
    const void* in;     // complex64, or items of the kernel's integer format
    size_t H;
    size_t seg0;        // the launch's first segment, counted from the call's
    const float4* G;    // [16][64]: the table in the lanes' order, components swapped
    const float4* tT;
    const cf* cc;
    cf* out;            // the call's samples
    uint32_t n_seg;     // segments of the launch
    uint32_t run;       // per wave
    uint32_t hop, V;
    float scale;        // of an integer format's unpack
};

// swap(a g) = conj(a) w for w = swap(g): (a.x w.x + a.y w.y, a.x w.y - a.y w.x).  cmul()'s pair of packed instructions
// with the sign on the other half (one statement, the product in the result register: see cmul)
__device__ __forceinline__ cf cmul_conj(cf a, cf w)
{
    cf r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]\n\t"
        "v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_hi:[1,0,0]"
        : "=&v"(r)
        : "v"(a), "v"(w));
    return r;
}

template <int F>
__global__ __launch_bounds__(kW64Threads, 2) void k_fft_filter(FilterArgs a)
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

    // segment `seg` of the launch begins at item (seg0 + seg) hop of tail ++ input
    auto load_half = [&](cf* dst, uint64_t seg, int h) {
        load_half_segment<F>(dst, a.hist, a.H, a.in, a.scale, (a.seg0 + seg) * a.hop, lane, h);
    };

    cf X[32];
    load_half(X, first, 0);
    load_half(X, first, 1);
    for (uint32_t s = 0; s < count; ++s) {
        // forward: the segment's bins, bin lane + 64 j in register j
        cf Z[32];
        dft32(X);
        w64_store(X, base);
        w64_mid_dev<1, true>(lane, row, ldsT, c, Z);
        // the table's rows, 16 KiB that stay in the L2: asked for in front of the last pass, used behind it
        int ln = lane;
        asm volatile("" : "+v"(ln)); // the address is formed here, not carried through the loop
        const float4* g = a.G + ln;
        float4 gq[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) gq[u] = g[64 * u];
        dft32(Z);
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            Z[2 * u] = cmul_conj(Z[2 * u], mk(gq[u].x, gq[u].y));
            Z[2 * u + 1] = cmul_conj(Z[2 * u + 1], mk(gq[u].z, gq[u].w));
        }
        // the same transform on swap(X G): swap(y_s)
        cf Y[32];
        dft32(Z);
        w64_store(Z, base);
        w64_mid_dev<1, true>(lane, row, ldsT, c, Y);
        // the first pass's registers are dead: they take the next segment -- one half now (it arrives while the last pass
        // runs), the other when that pass is complete (the pin: hipcc otherwise hoists those loads above the arithmetic)
        const bool has_next = s + 1 < count;
        if (has_next) load_half(X, first + s + 1, 0);
        dft32(Y);
#pragma unroll
        for (int k = 0; k < 32; k += 4) w64_pin4(Y + k);
        if (has_next) load_half(X, first + s + 1, 1);
        // sample p = lane + 64 j of the segment is out[(seg0 + first + s) hop + p - V] for p >= V (one address per lane,
        // formed in integers: it lies in front of `out` for the lanes of segment 0 that store nothing at small j)
        const int64_t at = static_cast<int64_t>((a.seg0 + first + s) * a.hop + lane) - static_cast<int64_t>(a.V);
        cf* o = reinterpret_cast<cf*>(reinterpret_cast<intptr_t>(a.out) + at * static_cast<int64_t>(sizeof(cf)));
#pragma unroll
        for (int j = 0; j < 32; ++j)
            if (static_cast<uint32_t>(lane + 64 * j) >= a.V) o[64 * j] = swap_xy(Y[j]);
    }
}

} // namespace

struct gr4pm_fft_filter {
    gr4pm::hostlogic::FftFilterShape shape = {};
    size_t n_taps = 0;
    uint64_t taken = 0; // samples since create or reset
    hipStream_t stream = nullptr;
    gr4pm::SegmentTransform tf; // the transform's tables and the waves of one launch (its window is not used)
    gr4pm::StreamTail tail;     // keep = V, frame = hop
    gr4pm::DevBuf<float4> d_G;  // [16][64]
    gr4pm::DevBuf<float2> d_zeros, d_last; // flush(): hop zeros to complete the last segment, and where it is written
    std::vector<float4> G_host;            // the table of the next upload (lives until the stream has read it)
};

namespace {

gr4pm_status sizes_error(FftFilterSizes e, size_t L, size_t V)
{
    switch (e) {
    case FftFilterSizes::ok: return GR4PM_OK;
    case FftFilterSizes::no_taps: set_error("fft_filter: no taps"); break;
    case FftFilterSizes::too_many_taps: set_error("fft_filter: %zu taps, at most %u", L, kFftFilterMaxTaps); break;
    case FftFilterSizes::overlap_short: set_error("fft_filter: overlap %zu is below n_taps - 1 = %zu", V, L - 1); break;
    case FftFilterSizes::overlap_long: set_error("fft_filter: overlap %zu, at most %u", V, kFftFilterMaxOverlap); break;
    }
    return GR4PM_ERR_INVALID;
}

gr4pm_status check_taps(const gr4pm_c64* taps, size_t L)
{
    if (!taps) {
        set_error("fft_filter: no taps array");
        return GR4PM_ERR_INVALID;
    }
    const size_t bad = fft_filter_first_bad_tap(reinterpret_cast<const float*>(taps), L);
    if (bad < L) {
        set_error("fft_filter: taps[%zu] is not finite", bad);
        return GR4PM_ERR_INVALID;
    }
    return GR4PM_OK;
}

// G[k] = (1 / N) sum_t h[t] exp(-2 pi j k t / N) in double (the phase k t mod N: exact), each component rounded to float
// once, in the kernel's layout with the components swapped
void make_table(const gr4pm_c64* taps, size_t L, std::vector<float4>& out)
{
    std::vector<double> cs(kN), sn(kN);
    for (size_t k = 0; k < kN; ++k) {
        const double ang = -2.0 * M_PI * static_cast<double>(k) / static_cast<double>(kN);
        cs[k] = std::cos(ang), sn[k] = std::sin(ang);
    }
    out.assign(16 * 64, float4{0, 0, 0, 0});
    for (size_t k = 0; k < kN; ++k) {
        double re = 0.0, im = 0.0;
        for (size_t t = 0; t < L; ++t) {
            const size_t ph = (k * t) % kN;
            const double hr = taps[t].re, hi = taps[t].im;
            re += hr * cs[ph] - hi * sn[ph];
            im += hr * sn[ph] + hi * cs[ph];
        }
        const float gr = static_cast<float>(re / static_cast<double>(kN)), gi = static_cast<float>(im / static_cast<double>(kN));
        const size_t lane = k % 64, j = k / 64;
        float4& q = out[(j / 2) * 64 + lane];
        if (j % 2 == 0)
            q.x = gi, q.y = gr;
        else
            q.z = gi, q.w = gr;
    }
}

// the launches of n_segments segments of tail ++ in; nothing is committed here
template <int F>
void launch_segments(const gr4pm_fft_filter& h, const StreamTail::Plan& t, const void* in, float scale, size_t n_segments, cf* out)
{
    FilterArgs a = {};
    a.hist = t.hist, a.in = in, a.H = t.H;
    a.G = h.d_G.p, a.tT = h.tf.d_tT.p, a.cc = h.tf.d_cc.p, a.out = out;
    a.hop = h.shape.hop, a.V = h.shape.overlap, a.scale = scale;
    for (size_t done = 0; done < n_segments;) {
        const size_t segs = std::min(n_segments - done, kChunk);
        const size_t per_wave = (segs + h.tf.max_waves - 1) / h.tf.max_waves;
        const size_t waves = (segs + per_wave - 1) / per_wave;
        a.seg0 = done, a.n_seg = static_cast<uint32_t>(segs), a.run = static_cast<uint32_t>(per_wave);
        hipLaunchKernelGGL(k_fft_filter<F>, dim3(static_cast<unsigned>((waves + kW64Waves - 1) / kW64Waves)), dim3(kW64Threads), 0,
                           h.stream, a);
        done += segs;
    }
}

// process() and process_iq(): format iq::kC64 for complex64 samples
gr4pm_status process_any(gr4pm_fft_filter* h, const void* in, int format, float scale, size_t n_in, gr4pm_c64* out, size_t out_cap,
                         size_t* n_out)
{
    if (!h || !n_out) return GR4PM_ERR_INVALID;
    *n_out = 0;
    if (!fft_filter_call_fits(n_in)) {
        set_error("fft_filter: %zu samples in one call, at most 2^40", n_in);
        return GR4PM_ERR_OVERFLOW;
    }
    if (n_in == 0) return GR4PM_OK;
    const FftFilterPlan p = fft_filter_plan(h->shape, h->taken, n_in);
    if (fft_filter_refuses(p, out_cap)) {
        set_error("fft_filter: %zu samples, room for %zu", p.samples, out_cap);
        return GR4PM_ERR_OVERFLOW;
    }
    if (!in || (p.samples && !out)) {
        set_error("fft_filter: no input or output array");
        return GR4PM_ERR_INVALID;
    }
    const StreamTail::Plan t = h->tail.plan(n_in); // H = V + carried, n_frames = the plan's segments
    iq::with_format(format, [&](auto f) {
        launch_segments<decltype(f)::value>(*h, t, in, scale, p.n_segments, reinterpret_cast<cf*>(out));
        h->tail.launch_history<decltype(f)::value>(t, in, 0, n_in, scale, h->stream);
    });
    GR4PM_HIP_TRY(hipGetLastError());
    h->tail.commit(t);
    h->taken += n_in;
    *n_out = p.samples;
    return GR4PM_OK;
}

gr4pm_status upload_table(gr4pm_fft_filter* h, const gr4pm_c64* taps, size_t L)
{
    // the last upload has read G_host before it is rewritten
    GR4PM_HIP_TRY(hipStreamSynchronize(h->stream));
    make_table(taps, L, h->G_host);
    GR4PM_TRY(h->d_G.upload(h->G_host.data(), h->G_host.size(), h->stream));
    h->n_taps = L;
    return GR4PM_OK;
}

} // namespace

extern "C" {

gr4pm_status gr4pm_band_filter_taps(const double* bands, size_t n_bands, int mode, size_t n_taps, double attenuation_db,
                                    gr4pm_c64* taps_out)
try {
    if (mode != GR4PM_BAND_STOP && mode != GR4PM_BAND_PASS) {
        set_error("band_filter_taps: mode %d is neither GR4PM_BAND_STOP nor GR4PM_BAND_PASS", mode);
        return GR4PM_ERR_INVALID;
    }
    if (!taps_out) {
        set_error("band_filter_taps: no output array");
        return GR4PM_ERR_INVALID;
    }
    std::vector<double> h;
    if (const char* e = band_filter_design(bands, n_bands, mode == GR4PM_BAND_PASS, n_taps, attenuation_db, h)) {
        set_error("band_filter_taps: %s", e);
        return GR4PM_ERR_INVALID;
    }
    for (size_t t = 0; t < n_taps; ++t) {
        taps_out[t].re = static_cast<float>(h[2 * t]);
        taps_out[t].im = static_cast<float>(h[2 * t + 1]);
    }
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_filter_create(const gr4pm_fft_filter_params* p, gr4pm_fft_filter** out)
try {
    if (!p || !out) return GR4PM_ERR_INVALID;
    *out = nullptr;
    GR4PM_TRY(sizes_error(fft_filter_check_sizes(p->n_taps, p->overlap), p->n_taps, p->overlap));
    GR4PM_TRY(check_taps(p->taps, p->n_taps));
    std::unique_ptr<gr4pm_fft_filter> h(new (std::nothrow) gr4pm_fft_filter);
    if (!h) return GR4PM_ERR_NOMEM;
    h->shape = fft_filter_shape(p->overlap ? static_cast<uint32_t>(p->overlap) : fft_filter_default_overlap(p->n_taps));
    h->stream = static_cast<hipStream_t>(p->stream);
    GR4PM_TRY(h->tf.create(nullptr, h->stream, "fft_filter"));
    GR4PM_TRY(h->d_G.alloc(16 * 64));
    GR4PM_TRY(h->d_zeros.alloc(h->shape.hop));
    GR4PM_TRY(h->d_last.alloc(h->shape.hop));
    GR4PM_TRY(h->d_zeros.zero(h->stream));
    GR4PM_TRY(h->tail.alloc(h->shape.overlap, h->shape.hop, 1, h->stream));
    GR4PM_TRY(upload_table(h.get(), p->taps, p->n_taps));
    return finish_create(h, out, "fft_filter");
}
GR4PM_ABI_CATCH

void gr4pm_fft_filter_destroy(gr4pm_fft_filter* h)
try {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    delete h;
}
GR4PM_ABI_CATCH_VOID

gr4pm_status gr4pm_fft_filter_reset(gr4pm_fft_filter* h)
try {
    if (!h) return GR4PM_ERR_INVALID;
    GR4PM_TRY(h->tail.reset(h->stream));
    h->taken = 0;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_filter_set_taps(gr4pm_fft_filter* h, const gr4pm_c64* taps, size_t n_taps)
try {
    if (!h) return GR4PM_ERR_INVALID;
    GR4PM_TRY(sizes_error(fft_filter_check_new_taps(n_taps, h->shape.overlap), n_taps, h->shape.overlap));
    GR4PM_TRY(check_taps(taps, n_taps));
    return upload_table(h, taps, n_taps);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_filter_sizes(const gr4pm_fft_filter* h, size_t* overlap, size_t* hop, size_t* n_taps)
try {
    if (!h || !overlap || !hop || !n_taps) return GR4PM_ERR_INVALID;
    *overlap = h->shape.overlap, *hop = h->shape.hop, *n_taps = h->n_taps;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_filter_pending(const gr4pm_fft_filter* h, size_t* samples)
try {
    if (!h || !samples) return GR4PM_ERR_INVALID;
    *samples = fft_filter_flush(h->shape, h->taken).owed;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_filter_output_items(const gr4pm_fft_filter* h, size_t n_in, size_t* n_out)
try {
    if (!h || !n_out) return GR4PM_ERR_INVALID;
    *n_out = 0;
    if (!fft_filter_call_fits(n_in)) {
        set_error("fft_filter: %zu samples in one call, at most 2^40", n_in);
        return GR4PM_ERR_OVERFLOW;
    }
    *n_out = fft_filter_plan(h->shape, h->taken, n_in).samples;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_filter_process(gr4pm_fft_filter* h, const gr4pm_c64* in, size_t n_in, gr4pm_c64* out, size_t out_cap,
                                      size_t* n_out)
try {
    return process_any(h, in, iq::kC64, 0.0f, n_in, out, out_cap, n_out);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_filter_process_iq(gr4pm_fft_filter* h, const void* in, int format, float scale, size_t n_in, gr4pm_c64* out,
                                         size_t out_cap, size_t* n_out)
try {
    if (!h || !n_out) return GR4PM_ERR_INVALID;
    *n_out = 0;
    if (!iq::valid(format)) {
        set_error("fft_filter: format %d is none of GR4PM_IQ_SC16 / SC8 / CU8", format);
        return GR4PM_ERR_INVALID;
    }
    return process_any(h, in, format, scale == 0.0f ? iq::default_scale(format) : scale, n_in, out, out_cap, n_out);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_filter_flush(gr4pm_fft_filter* h, gr4pm_c64* out, size_t out_cap, size_t* n_out)
try {
    if (!h || !n_out) return GR4PM_ERR_INVALID;
    *n_out = 0;
    const FftFilterFlush f = fft_filter_flush(h->shape, h->taken);
    if (f.owed > out_cap) {
        set_error("fft_filter: flush owes %zu samples, room for %zu", f.owed, out_cap);
        return GR4PM_ERR_OVERFLOW;
    }
    if (f.owed && !out) {
        set_error("fft_filter: no output array");
        return GR4PM_ERR_INVALID;
    }
    if (f.owed) {
        // the last segment over zeros, whole, into the handle's own buffer; its first `owed` kept samples to the caller
        const StreamTail::Plan t = h->tail.plan(f.zeros);
        launch_segments<iq::kC64>(*h, t, h->d_zeros.p, 0.0f, 1, reinterpret_cast<cf*>(h->d_last.p));
        GR4PM_HIP_TRY(hipGetLastError());
        GR4PM_HIP_TRY(hipMemcpyAsync(out, h->d_last.p, f.owed * sizeof(float2), hipMemcpyDeviceToDevice, h->stream));
    }
    GR4PM_TRY(h->tail.reset(h->stream));
    h->taken = 0;
    *n_out = f.owed;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

} // extern "C"
