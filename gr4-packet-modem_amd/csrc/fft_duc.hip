// fft_duc.hip -- K carriers onto one wideband stream from one shared transform: the fast-convolution (overlap-save) form
// of the Duc for power-of-two interpolations, the mirror of fft_ddc.hip.  The project's own block (the reference is a
// one-channel modem).  Definition (include/gr4pm_hip.h; the integer side is
// hostlogic/fft_duc_plan.hpp's):
//     N = 2048, B = N / I, hop = N - V, segment s = the N output samples from a_s = s hop - V on, made of the B items
//     m = a_s / I + n' of every row, v = 0 before the start
//     z_k[m] = q_k[m] v_k[m]  (the Duc's rotator),  Z_k = FFT_B(z_k over the segment)
//     S[b] = sum_k G_k[u] Z_k[b mod B],  b = (c_k + u) mod N,  u in [-R B / 2, R B / 2)   (from zero, k ascending)
//     x[p] = sum_b S[b] exp(+2 pi j b p / N),  p = V .. N - 1 kept:  out[s hop + p - V] = x[p]
//
// Two kernels, with the segments' whole spectra between them:
// k_fft_duc_assemble: one workgroup of four waves per segment, the segment's 2048 bins in LDS.  The channels go through in
//   groups of four, a wave each: the wave stages the B items of its row from the carried items or the input, rotated on
//   the way in (one double sincospi per staged item, four fmaf from zero), and runs log2 B radix-2 autosort (Stockham)
//   stages between two LDS buffers of its own, natural order in and out, twiddles exp(-2 pi j m / 512) from a table made
//   in double: section 25's loop with the conjugate twiddles, with wave-level synchronisation only, since no other wave
//   touches the buffers.  Behind one barrier all 256 threads add the group's channels to the bins, one channel after the
//   other in ascending k with a barrier between them: thread t takes the table's items t, t + 256, ..., which are
//   different bins (R B <= N), so within a channel no two threads meet and across channels the barrier orders them.
//   Whoever adds to a bin has seen all its earlier channels: no atomics, and the slices may overlap and wrap bin 0.
//   The bins leave as spec[segment][2048].
// k_fft_duc_inverse: k_fft_ddc_forward's wave on the one-exchange transform of fft2048_w64.hpp, whose input and output
//   layouts are the same (register j of lane l is item / bin l + 64 j).  It reads a spectrum with real and imaginary
//   parts swapped, transforms forward and swaps back: the exact inverse, j conj(F(j conj S)) = F^-1(S) N, with no new
//   transform.  Only the samples p >= V are stored.
// A launch pair covers at most kChunk segments, so the spectra of a call of any length stay within one 64 MiB buffer
// that the next pair reuses in stream order.  No atomics, no scratch; a segment's samples are a function of its B items
// per row, the tables and its index only, whatever the cuts into calls.
// Built with FFT_FLAGS: the transforms and the products may contract to FMA.  The rotator is written in explicit fmaf
// (freq_xlate.hpp's cmac), so it is the Duc's under either set of flags.
#include "spectrum_segment.hpp"
#include "freq_xlate.hpp"
#include "hostlogic/fft_duc_plan.hpp"

#include <algorithm>
#include <cmath>

namespace {

namespace iq = gr4pm::iq;
using namespace gr4pm;
using gr4pm::hostlogic::fft_ddc_bin;
using gr4pm::hostlogic::fft_ddc_pow2;
using gr4pm::hostlogic::fft_ddc_table_word;
using gr4pm::hostlogic::fft_duc_default_overlap;
using gr4pm::hostlogic::fft_duc_item_index;
using gr4pm::hostlogic::fft_duc_plan;
using gr4pm::hostlogic::fft_duc_shape;
using gr4pm::hostlogic::fft_duc_validate;
using gr4pm::hostlogic::FftDucPlan;
using gr4pm::hostlogic::FftDucRefusal;
using gr4pm::hostlogic::FftDucShape;
using gr4pm::hostlogic::kFftDucMaxI;
using gr4pm::hostlogic::kFftDucMaxK;
using gr4pm::hostlogic::kFftDucMinHop;
using gr4pm::hostlogic::kFftDucMinI;

constexpr size_t kN = kFftN;
constexpr size_t kChunk = 4096;  // segments of one launch pair: 64 MiB of spectra
constexpr int kTwiddles = 256;   // exp(-2 pi j m / 512), m < 256
constexpr int kAsmWaves = 4, kAsmThreads = kAsmWaves * 64;

struct AsmArgs {
    const float2* hist; // [K][H]: the items in front of in[k][0]
    const float2* in;   // row k at in + k in_stride
    size_t in_stride;
    size_t H;
    size_t seg0;        // the launch's first segment, counted from the call's
    const float2* G;    // [K][R B]: item t is u = t - R B / 2
    const float2* tw;   // [256]
    const uint32_t* w;  // [K] frequency words
    float2* spec;       // [segments of the launch][2048]
    uint32_t index0;    // absolute index of the first input item of the launch's first segment (its low 32 bits)
    uint32_t K, I, logB, R;
    uint32_t hop, hop_items;
};

// what the lanes of one wave wrote to LDS is visible to its other lanes behind this: no workgroup barrier where a wave
// works in buffers of its own
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// blockIdx.x: the segment of the launch; kAsmThreads threads; dynamic LDS: tw[256] | S[2048] | per wave two buffers of B
// items
__global__ __launch_bounds__(kAsmThreads) void k_fft_duc_assemble(AsmArgs a)
{
    extern __shared__ float2 s_fft_duc[];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t B = 1u << a.logB, RB = a.R << a.logB;
    float2* tw = s_fft_duc;
    float2* S = s_fft_duc + kTwiddles;
    float2* bufs = S + kN;
    float2* mine = bufs + wave * 2 * B;
    for (uint32_t m = tid; m < kTwiddles; m += kAsmThreads) tw[m] = a.tw[m];
    for (uint32_t b = tid; b < kN; b += kAsmThreads) S[b] = float2{0.0f, 0.0f};
    __syncthreads();

    const uint32_t seg = blockIdx.x;
    const size_t v0 = (a.seg0 + seg) * a.hop_items; // the segment's first item of a row's carried ++ input
    const uint32_t i0 = a.index0 + seg * a.hop;
    const uint32_t src = a.logB & 1;                // the buffer that holds a transform's result

    for (uint32_t k0 = 0; k0 < a.K; k0 += kAsmWaves) {
        const uint32_t k = k0 + wave;
        if (k < a.K) { // uniform over the wave, which works in its own two buffers up to the barrier below
            const uint32_t wk = a.w[k];
            const float2* hist = a.hist + static_cast<size_t>(k) * a.H;
            const float2* in = a.in + static_cast<size_t>(k) * a.in_stride;
            for (uint32_t n = lane; n < B; n += 64) {
                const size_t v = v0 + n;
                const float2 x = v < a.H ? hist[v] : in[v - a.H];
                float2 z = {0.0f, 0.0f};
                cmac(z, mixer<1>(wk, i0 + n * a.I), x);
                mine[n] = z;
            }
            wave_sync();
            // stage of sub-transform length Ns: butterfly j takes items j and j + B / 2, position q = j mod Ns of its
            // sub-transform, and writes items (j - q) 2 + q and Ns later.  Natural order in, natural order out
            for (uint32_t ls = 0; ls < a.logB; ++ls) {
                const uint32_t Ns = 1u << ls;
                const float2* from = mine + (ls & 1) * B;
                float2* to = mine + ((ls & 1) ^ 1) * B;
                for (uint32_t j = lane; j < B / 2; j += 64) {
                    const uint32_t q = j & (Ns - 1);
                    const float2 t = tw[q << (8 - ls)]; // exp(-2 pi j q / (2 Ns))
                    const float2 p = from[j], b = from[j + B / 2];
                    const float2 e = {b.x * t.x - b.y * t.y, b.x * t.y + b.y * t.x};
                    const uint32_t o2 = ((j - q) << 1) + q;
                    to[o2] = float2{p.x + e.x, p.y + e.y};
                    to[o2 + Ns] = float2{p.x - e.x, p.y - e.y};
                }
                wave_sync();
            }
        }
        __syncthreads();

        // the group's channels into the segment's bins, k ascending: thread t takes the table's items t, t + 256, ..., which
        // are different bins; the barrier orders a bin's channels
        const uint32_t gc = a.K - k0 < kAsmWaves ? a.K - k0 : kAsmWaves;
        for (uint32_t kk = 0; kk < gc; ++kk) {
            const uint32_t c = fft_ddc_bin(a.w[k0 + kk]);
            const float2* Z = bufs + (kk * 2 + src) * B;
            const float2* __restrict__ Gk = a.G + static_cast<size_t>(k0 + kk) * RB;
            const uint32_t bin0 = c + static_cast<uint32_t>(kN) - RB / 2; // bin of the table's item 0, before the wrap
            for (uint32_t t = tid; t < RB; t += kAsmThreads) {
                const uint32_t b = (bin0 + t) & (kN - 1);
                const float2 g = Gk[t], z = Z[b & (B - 1)];
                float2 s = S[b];
                s.x += g.x * z.x - g.y * z.y;
                s.y += g.x * z.y + g.y * z.x;
                S[b] = s;
            }
            __syncthreads(); // behind the last channel: the buffers take the next group
        }
    }

    float2* o = a.spec + static_cast<size_t>(seg) * kN;
    for (uint32_t b = tid; b < kN; b += kAsmThreads) o[b] = S[b];
}

struct InvArgs {
    const cf* spec; // [segments of the launch][2048]
    const float4* tT;
    const cf* cc;
    cf* out;        // the call's samples
    size_t seg0;    // the launch's first segment, counted from the call's
    uint32_t n_seg; // segments of the launch
    uint32_t run;   // per wave
    uint32_t hop, V;
};

__global__ __launch_bounds__(kW64Threads, 2) void k_fft_duc_inverse(InvArgs a)
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

    // half h of the launch's segment `seg`: bins lane + 64 j, j = 16 h .. 16 h + 15, real and imaginary parts swapped
    auto load_half = [&](cf* dst, uint64_t seg, int h) {
        const cf* x = a.spec + seg * kN + lane;
#pragma unroll
        for (int j = 16 * h; j < 16 * h + 16; ++j) dst[j] = swap_xy(x[64 * j]);
    };

    cf X[32];
    load_half(X, first, 0);
    load_half(X, first, 1);
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
        cf* o = reinterpret_cast<cf*>(reinterpret_cast<intptr_t>(a.out) + at * static_cast<int64_t>(sizeof(cf)));
#pragma unroll
        for (int j = 0; j < 32; ++j)
            if (static_cast<uint32_t>(lane + 64 * j) >= a.V) o[64 * j] = swap_xy(bq[j]);
    }
}

// G_k[u] = (a_k / N) sum_t h[t] exp(-2 pi j psi t / 2^32), psi = ((c_k + u) 2^21 - w_k) mod 2^32: the FftDdc's table times
// the gain; the phase of every term an exact integer, the sum in double, each component rounded to float once
float2 response(const std::vector<float>& h, double gain, uint32_t w, uint32_t c, int32_t u)
{
    const uint32_t psi = fft_ddc_table_word(w, c, u);
    double re = 0.0, im = 0.0;
    for (size_t t = 0; t < h.size(); ++t) {
        double cs, sn;
        unit_phasor(0u - psi * static_cast<uint32_t>(t), cs, sn);
        re += static_cast<double>(h[t]) * cs;
        im += static_cast<double>(h[t]) * sn;
    }
    const double scale = gain / static_cast<double>(kN);
    return float2{static_cast<float>(scale * re), static_cast<float>(scale * im)};
}

gr4pm_status check_interpolation(size_t I)
{
    if (!fft_ddc_pow2(I) || I < kFftDucMinI || I > kFftDucMaxI) {
        set_error("fft_duc: the interpolation must be a power of two in [%u, %u], not %zu", kFftDucMinI, kFftDucMaxI, I);
        return GR4PM_ERR_INVALID;
    }
    return GR4PM_OK;
}

// dynamic LDS of k_fft_duc_assemble
size_t assemble_lds(size_t I) { return (kTwiddles + kN + kAsmWaves * 2 * (kN / I)) * sizeof(float2); }

gr4pm_status check_items(size_t n_in)
{
    if (n_in > (size_t(1) << 40)) {
        set_error("fft_duc: %zu items per row in one call, at most 2^40", n_in);
        return GR4PM_ERR_OVERFLOW;
    }
    return GR4PM_OK;
}

} // namespace

struct gr4pm_fft_duc {
    size_t K = 0, I = 0, R = 0, V = 0;
    uint64_t start_index = 0;
    uint64_t taken = 0; // items per row since create or reset
    FftDucShape shape = {};
    hipStream_t stream = nullptr;
    size_t max_waves = 2048; // of one inverse launch: eight per compute unit, at most 2048
    gr4pm::StreamTail tail;  // keep = V / I, frame = hopI, K rows
    std::vector<uint32_t> words;
    gr4pm::DevBuf<float4> d_tT;
    gr4pm::DevBuf<cf> d_cc, d_spec;
    gr4pm::DevBuf<float2> d_tw, d_G;
    gr4pm::DevBuf<uint32_t> d_w;
};

extern "C" {

gr4pm_status gr4pm_fft_duc_taps(size_t interpolation, size_t taps_per_phase, float* out)
try {
    if (!out) return GR4PM_ERR_INVALID;
    GR4PM_TRY(check_interpolation(interpolation));
    return gr4pm_duc_taps(interpolation, taps_per_phase, 0.25, 0.75, out);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_duc_create(const gr4pm_fft_duc_params* p, gr4pm_fft_duc** out)
try {
    if (!p || !out) return GR4PM_ERR_INVALID;
    *out = nullptr;
    const size_t K = p->n_channels, I = p->interpolation, R = p->images;
    std::vector<uint32_t> words;
    GR4PM_TRY(frequency_words("fft_duc", p->frequencies, K, kFftDucMaxK, words));
    GR4PM_TRY(check_interpolation(I));
    GR4PM_TRY(finite_gains("fft_duc", p->gains, K));
    if (!fft_ddc_pow2(R) || R > I) {
        set_error("fft_duc: images must be a power of two in [1, %zu], not %zu", I, R);
        return GR4PM_ERR_INVALID;
    }
    GR4PM_TRY(prototype_length("fft_duc", p->taps, p->n_taps, kN));
    std::vector<float> taps;
    if (p->taps) {
        taps.assign(p->taps, p->taps + p->n_taps);
    } else {
        if (p->taps_per_phase < 1 || p->taps_per_phase * I > kN) {
            set_error("fft_duc: %zu taps per phase at an interpolation of %zu: the prototype has 1 .. %zu taps", p->taps_per_phase, I, kN);
            return GR4PM_ERR_INVALID;
        }
        taps.resize(p->taps_per_phase * I);
        GR4PM_TRY(gr4pm_duc_taps(I, p->taps_per_phase, 0.25, 0.75, taps.data()));
    }
    const size_t L = taps.size();
    for (size_t t = 0; t < L; ++t)
        if (!std::isfinite(taps[t])) {
            set_error("fft_duc: taps[%zu] is not finite", t);
            return GR4PM_ERR_INVALID;
        }
    const size_t V = p->overlap < 0 ? fft_duc_default_overlap(L) : static_cast<size_t>(p->overlap);
    switch (fft_duc_validate(K, I, R, L, V)) {
    case FftDucRefusal::none: break;
    case FftDucRefusal::overlap_multiple:
        set_error("fft_duc: the overlap %zu is no multiple of the interpolation %zu", V, I);
        return GR4PM_ERR_INVALID;
    case FftDucRefusal::overlap_low:
        set_error("fft_duc: the overlap %zu is below the %zu taps' reach of %zu samples", V, L, L - 1);
        return GR4PM_ERR_INVALID;
    case FftDucRefusal::overlap_high:
        set_error("fft_duc: the overlap %zu leaves a hop below %u: at most %zu", V, kFftDucMinHop, kN - kFftDucMinHop);
        return GR4PM_ERR_INVALID;
    default: set_error("fft_duc: invalid sizes"); return GR4PM_ERR_INVALID;
    }
    GR4PM_TRY(require_device());
    std::unique_ptr<gr4pm_fft_duc> h(new (std::nothrow) gr4pm_fft_duc);
    if (!h) return GR4PM_ERR_NOMEM;
    h->K = K, h->I = I, h->R = R, h->V = V;
    h->start_index = p->start_index;
    h->shape = fft_duc_shape(static_cast<uint32_t>(I), static_cast<uint32_t>(V));
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
        unit_phasor(0u - (static_cast<uint32_t>(m) << 23), cs, sn); // -m / 512 of a turn
        tw[m] = float2{static_cast<float>(cs), static_cast<float>(sn)};
    }
    const size_t B = kN / I, RB = R * B;
    std::vector<float2> G(K * RB);
    for (size_t k = 0; k < K; ++k) {
        const uint32_t w = h->words[k], c = fft_ddc_bin(w);
        const double gain = p->gains ? p->gains[k] : 1.0;
        for (size_t t = 0; t < RB; ++t) G[k * RB + t] = response(taps, gain, w, c, static_cast<int32_t>(t) - static_cast<int32_t>(RB / 2));
    }
    GR4PM_TRY(h->d_tT.alloc(tT.size()));
    GR4PM_TRY(h->d_cc.alloc(cc.size()));
    GR4PM_TRY(h->d_tw.alloc(tw.size()));
    GR4PM_TRY(h->d_spec.alloc(kChunk * kN));
    GR4PM_TRY(h->d_G.alloc(G.size()));
    GR4PM_TRY(h->d_w.alloc(K));
    GR4PM_TRY(h->d_tT.upload(tT.data(), tT.size(), h->stream));
    GR4PM_TRY(h->d_cc.upload(cc.data(), cc.size(), h->stream));
    GR4PM_TRY(h->d_tw.upload(tw.data(), tw.size(), h->stream));
    GR4PM_TRY(h->d_G.upload(G.data(), G.size(), h->stream));
    GR4PM_TRY(h->d_w.upload(h->words.data(), K, h->stream));
    GR4PM_TRY(h->tail.alloc(h->shape.keep, h->shape.hop_items, K, h->stream));
    if (assemble_lds(I) > 48 * 1024) // B = 512
        GR4PM_TRY(raise_dynamic_lds({reinterpret_cast<const void*>(&k_fft_duc_assemble)}, assemble_lds(I), "fft_duc"));
    return finish_create(h, out, "fft_duc"); // waits for the stream: the uploads read this function's vectors
}
GR4PM_ABI_CATCH

void gr4pm_fft_duc_destroy(gr4pm_fft_duc* h)
try {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    delete h;
}
GR4PM_ABI_CATCH_VOID

gr4pm_status gr4pm_fft_duc_reset(gr4pm_fft_duc* h)
try {
    if (!h) return GR4PM_ERR_INVALID;
    GR4PM_TRY(h->tail.reset(h->stream));
    h->taken = 0;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_duc_output_items(const gr4pm_fft_duc* h, size_t n_in, size_t* n_out)
try {
    if (!h || !n_out) return GR4PM_ERR_INVALID;
    *n_out = 0;
    GR4PM_TRY(check_items(n_in));
    *n_out = fft_duc_plan(h->shape, h->taken, n_in).samples;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_duc_frequencies(const gr4pm_fft_duc* h, double* out)
try {
    if (!h || !out) return GR4PM_ERR_INVALID;
    for (size_t k = 0; k < h->K; ++k) out[k] = folded_frequency(h->words[k]);
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_duc_sizes(const gr4pm_fft_duc* h, size_t* overlap, size_t* hop)
try {
    if (!h || !overlap || !hop) return GR4PM_ERR_INVALID;
    *overlap = h->V;
    *hop = h->shape.hop;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_duc_pending(const gr4pm_fft_duc* h, size_t* items)
try {
    if (!h || !items) return GR4PM_ERR_INVALID;
    *items = static_cast<size_t>(h->taken % h->shape.hop_items);
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_duc_process(gr4pm_fft_duc* h, const gr4pm_c64* in, size_t in_stride, size_t n_in, gr4pm_c64* out,
                                   size_t out_cap, size_t* n_out)
try {
    if (!h || !n_out) return GR4PM_ERR_INVALID;
    *n_out = 0;
    GR4PM_TRY(check_items(n_in));
    if (n_in == 0) return GR4PM_OK;
    const FftDucPlan p = fft_duc_plan(h->shape, h->taken, n_in);
    if (p.samples > out_cap) {
        set_error("fft_duc: %zu samples, room for %zu", p.samples, out_cap);
        return GR4PM_ERR_OVERFLOW;
    }
    if (!in || (p.samples && !out) || (h->K > 1 && in_stride < n_in)) {
        set_error("fft_duc: no input or output array, or a row stride of %zu items for %zu items", in_stride, n_in);
        return GR4PM_ERR_INVALID;
    }
    const StreamTail::Plan t = h->tail.plan(n_in); // H = p.carried, n_frames = p.n_segments, H_new = p.left
    AsmArgs a = {};
    a.hist = t.hist, a.in = reinterpret_cast<const float2*>(in), a.in_stride = in_stride, a.H = t.H;
    a.G = h->d_G.p, a.tw = h->d_tw.p, a.w = h->d_w.p, a.spec = reinterpret_cast<float2*>(h->d_spec.p);
    a.K = static_cast<uint32_t>(h->K), a.I = static_cast<uint32_t>(h->I), a.R = static_cast<uint32_t>(h->R);
    a.logB = static_cast<uint32_t>(__builtin_ctzll(kN / h->I));
    a.hop = h->shape.hop, a.hop_items = h->shape.hop_items;
    InvArgs b = {};
    b.spec = h->d_spec.p, b.tT = h->d_tT.p, b.cc = h->d_cc.p, b.out = reinterpret_cast<cf*>(out);
    b.hop = h->shape.hop, b.V = static_cast<uint32_t>(h->V);
    const size_t lds = assemble_lds(h->I);
    for (size_t done = 0; done < p.n_segments;) {
        const size_t segs = std::min(p.n_segments - done, kChunk);
        a.seg0 = done;
        a.index0 = static_cast<uint32_t>(fft_duc_item_index(h->shape, h->start_index, p.segments_before + done));
        hipLaunchKernelGGL(k_fft_duc_assemble, dim3(static_cast<unsigned>(segs)), dim3(kAsmThreads), lds, h->stream, a);
        const size_t per_wave = (segs + h->max_waves - 1) / h->max_waves;
        const size_t waves = (segs + per_wave - 1) / per_wave;
        b.seg0 = done, b.n_seg = static_cast<uint32_t>(segs), b.run = static_cast<uint32_t>(per_wave);
        hipLaunchKernelGGL(k_fft_duc_inverse, dim3(static_cast<unsigned>((waves + kW64Waves - 1) / kW64Waves)), dim3(kW64Threads), 0,
                           h->stream, b);
        done += segs;
    }
    h->tail.launch_history<iq::kC64>(t, in, in_stride, n_in, 0.0f, h->stream);
    GR4PM_HIP_TRY(hipGetLastError());
    h->tail.commit(t);
    h->taken += n_in;
    *n_out = p.samples;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

} // extern "C"
