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
// k_fft_ddc_mixed: one wave per (segment, channel), with B, R, the kept items and the row from a per-channel descriptor
//   (k_fft_ddc_channel: the same body with them from the launch, for a bank whose channels are all alike).
//   Lane l takes the folded bins v = l, l + 64, ...: R products X[(c + u) mod N] G[u] in ascending u, consecutive lanes on
//   consecutive bins of the spectrum and of the table.  The B-point inverse transform is log2 B radix-2 autosort
//   (Stockham) stages between two LDS buffers, natural order in and out, twiddles exp(+2 pi j m / 512) from a table made
//   in double; then the kept items n' >= first take the rotator (the Ddc's: double sincospi of the exact phase, rounded
//   to float, four fmaf from zero) and leave as hop / D consecutive frames of row k.
// A launch pair covers at most kChunk segments, so the spectra of a call of any length stay within one 64 MiB buffer
// that the next pair reuses in stream order.  No atomics, no scratch; every result is a function of (channel, frame,
// stream) only, whatever the cuts into calls.
// One handle (FftDdcBank), one create and one call serve both ABI types.  The MixedFftDdc gives every
// channel its own D_k on the segment grid of Dmax; the FftDdc is the bank whose decimations are all equal, built by
// gr4pm_fft_ddc_create from its scalars: Dmax = D, first = V / D, frames = hop / D, no zeros behind a row, and the
// descriptors in channel order.  The call picks the channel kernel by what the bank holds, not by its ABI type.
// Built with FFT_FLAGS: the transforms, the products and the fold may contract to FMA.  The rotator is written in
// explicit fmaf (freq_xlate.hpp's cmac), so it is the Ddc's under either set of flags.
#include "spectrum_segment.hpp"
#include "freq_xlate.hpp"
#include "hostlogic/fft_ddc_plan.hpp"
#include "hostlogic/fft_ddc_mixed_plan.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

namespace {

namespace iq = gr4pm::iq;
using namespace gr4pm;
using gr4pm::hostlogic::fft_ddc_bin;
using gr4pm::hostlogic::fft_ddc_mixed_channel;
using gr4pm::hostlogic::fft_ddc_mixed_default_overlap;
using gr4pm::hostlogic::fft_ddc_mixed_frames;
using gr4pm::hostlogic::fft_ddc_mixed_max_decimation;
using gr4pm::hostlogic::fft_ddc_mixed_table_offsets;
using gr4pm::hostlogic::fft_ddc_mixed_validate;
using gr4pm::hostlogic::fft_ddc_mixed_validate_channels;
using gr4pm::hostlogic::fft_ddc_phi;
using gr4pm::hostlogic::fft_ddc_plan;
using gr4pm::hostlogic::fft_ddc_pow2;
using gr4pm::hostlogic::fft_ddc_segment_index;
using gr4pm::hostlogic::fft_ddc_shape;
using gr4pm::hostlogic::fft_ddc_table_word;
using gr4pm::hostlogic::FftDdcMixedChannel;
using gr4pm::hostlogic::FftDdcMixedRefusal;
using gr4pm::hostlogic::FftDdcMixedVerdict;
using gr4pm::hostlogic::FftDdcPlan;
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

// One wave's work for a (segment, channel), the arithmetic of both channel kernels: X the segment's spectrum, G the
// channel's table (item t is u = t - R B / 2), w its frequency word, B = 2^logB; the items n' = first .. first + frames - 1 of the inverse
// transform leave as o[0 .. frames - 1]; i0: the absolute index of the segment's item 0 (its low 32 bits).
__device__ __forceinline__ void fft_ddc_channel_body(const float2* __restrict__ twg, const float2* __restrict__ X,
                                                     const float2* __restrict__ G, const uint32_t* __restrict__ w, uint32_t logB, uint32_t R, uint32_t first,
                                                     uint32_t D, uint32_t frames, uint32_t i0, float2* __restrict__ o)
{
    __shared__ float2 buf[2][kMaxB];
    __shared__ float2 tw[kTwiddles];
    const uint32_t lane = threadIdx.x;
    const uint32_t B = 1u << logB, RB = R << logB;
    for (uint32_t m = lane; m < kTwiddles; m += 64) tw[m] = twg[m];

    const uint32_t wk = *w, c = fft_ddc_bin(wk);
    const uint32_t bin0 = c + static_cast<uint32_t>(kN) - RB / 2; // bin of the table's item 0, before the wrap
    for (uint32_t v = lane; v < B; v += 64) {
        uint32_t t = (v + RB / 2) & (B - 1); // the table's first item of the folded bin v; the others are B apart
        float2 y = {0.0f, 0.0f};
        for (uint32_t r = 0; r < R; ++r, t += B) {
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
    for (uint32_t ls = 0; ls < logB; ++ls) {
        const uint32_t Ns = 1u << ls;
        for (uint32_t j = lane; j < B / 2; j += 64) {
            const uint32_t q = j & (Ns - 1);
            const float2 t = tw[q << (8 - ls)]; // exp(+2 pi j q / (2 Ns))
            const float2 p = buf[src][j], b = buf[src][j + B / 2];
            const float2 e = {b.x * t.x - b.y * t.y, b.x * t.y + b.y * t.x};
            const uint32_t o2 = ((j - q) << 1) + q;
            buf[src ^ 1][o2] = float2{p.x + e.x, p.y + e.y};
            buf[src ^ 1][o2 + Ns] = float2{p.x - e.x, p.y - e.y};
        }
        src ^= 1;
        __syncthreads();
    }

    for (uint32_t f = lane; f < frames; f += 64) {
        const uint32_t p = (first + f) * D;
        const uint32_t phi = fft_ddc_phi(wk, c, i0 + p, p);
        float2 y = {0.0f, 0.0f};
        cmac(y, mixer<-1>(phi, 1u), buf[src][first + f]);
        o[f] = y;
    }
}

// What the channel kernel takes per channel in the place of launch-wide constants.  The table is ordered by
// descending B, so the workgroups with the longest inverse transforms are dispatched first.
struct MixedDesc {
    uint32_t w;      // the frequency word
    uint32_t logB;   // log2 B_k
    uint32_t R;      // images
    uint32_t first;  // the first n' that is kept
    uint32_t D;      // D_k
    uint32_t frames; // hop / D_k
    uint32_t table;  // the channel's first item of G
    uint32_t row;    // the output row
};

// A bank whose channels all have one D and one R: what the descriptors say is the same for every channel, and goes with
// the launch (measured: a uniform K = 24 is 0.3 to 0.6 % faster this way, and K = 64 another 0.4 to 0.9 % with the words
// packed and not 32 bytes apart in the descriptors: profiles/fft_ddc_bench.txt).  The tables are R B items apart then.
struct ChanArgs {
    const float2* spec;    // [segments of the launch][2048]
    const float2* G;       // [K][R B]: item t is u = t - R B / 2
    const float2* tw;      // [256]
    const uint32_t* w;     // [K] frequency words, packed: a workgroup's first load, and 64 of them are four cache lines
    float2* out;
    size_t out_stride;
    size_t frame0;         // the launch's first frame of the call's rows
    uint64_t index0;       // absolute index of item 0 of the launch's first segment
    uint32_t D, logB, R;
    uint32_t first;        // V / D
    uint32_t hop;
};

// blockIdx.x: the segment of the launch, blockIdx.y: the channel; 64 threads.  The body is k_fft_ddc_mixed's below, so the
// bits are
__global__ __launch_bounds__(64) void k_fft_ddc_channel(ChanArgs a)
{
    const uint32_t seg = blockIdx.x, k = blockIdx.y;
    const uint32_t B = 1u << a.logB, RB = a.R << a.logB;
    const uint32_t frames = B - a.first;
    fft_ddc_channel_body(a.tw, a.spec + static_cast<size_t>(seg) * kN, a.G + static_cast<size_t>(k) * RB, a.w + k, a.logB, a.R, a.first, a.D,
                         frames, static_cast<uint32_t>(a.index0) + seg * a.hop,
                         a.out + static_cast<size_t>(k) * a.out_stride + a.frame0 + static_cast<size_t>(seg) * frames);
}

struct MixedArgs {
    const float2* spec;    // [segments of the launch][2048]
    const float2* G;       // the channels' tables behind one another, R_k B_k items each
    const float2* tw;      // [256]
    const MixedDesc* desc; // [K]
    float2* out;
    size_t out_stride;
    size_t seg0;           // the launch's first segment, counted from the call's
    size_t call_segments;  // segments of the call
    uint64_t index0;       // absolute index of item 0 of the launch's first segment
    uint32_t hop;
    uint32_t max_frames;   // hop / min D_k: frames of a segment on the longest row
};

// blockIdx.x: the segment of the launch, blockIdx.y: the descriptor; 64 threads.  Row k takes the call's frames_k frames
// per segment from the front; behind the call's last frame the workgroup of the call's segment s writes the zeros
// [s (max_frames - frames_k), (s + 1) (max_frames - frames_k)), so all rows end at call_segments max_frames
__global__ __launch_bounds__(64) void k_fft_ddc_mixed(MixedArgs a)
{
    const uint32_t seg = blockIdx.x;
    const MixedDesc d = a.desc[blockIdx.y];
    const size_t s = a.seg0 + seg;
    float2* __restrict__ row = a.out + static_cast<size_t>(d.row) * a.out_stride;
    fft_ddc_channel_body(a.tw, a.spec + static_cast<size_t>(seg) * kN, a.G + d.table, &a.desc[blockIdx.y].w, d.logB, d.R, d.first, d.D, d.frames,
                         static_cast<uint32_t>(a.index0) + seg * a.hop, row + s * d.frames);
    const uint32_t pad = a.max_frames - d.frames;
    float2* __restrict__ z = row + a.call_segments * d.frames + s * pad;
    for (uint32_t f = threadIdx.x; f < pad; f += 64) z[f] = float2{0.0f, 0.0f};
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

// The one handle behind both ABI types: K channels with a decimation each on the segment grid of (Dmax, V).  An FftDdc is
// the bank whose decimations are all equal: Dmax = D, every row takes shape.frames frames a segment and no zeros follow.
struct FftDdcBank {
    virtual ~FftDdcBank() = default; // the ABI types derive from it and are deleted through it
    const char* name = ""; // of the entry points' messages: fft_ddc or fft_ddc_mixed
    size_t K = 0, V = 0;
    uint32_t max_frames = 0; // hop / min D_k
    MixedDesc alike = {};    // a channel's sizes where all channels have one D and one R (logB != 0 then): k_fft_ddc_channel serves
    uint64_t start_index = 0;
    uint64_t taken = 0; // samples since create or reset
    FftDdcShape shape = {}; // of (Dmax, V)
    hipStream_t stream = nullptr;
    size_t max_waves = 2048; // of one forward launch: eight per compute unit, at most 2048
    gr4pm::StreamTail tail; // keep = 0, frame = N: the virtual items of the incomplete segment
    std::vector<uint32_t> words;
    std::vector<FftDdcMixedChannel> channels;
    gr4pm::DevBuf<float4> d_tT;
    gr4pm::DevBuf<cf> d_cc, d_spec;
    gr4pm::DevBuf<float2> d_tw, d_G;
    gr4pm::DevBuf<MixedDesc> d_desc;
    gr4pm::DevBuf<uint32_t> d_w; // the words again, packed, for k_fft_ddc_channel
};

// The create of both handles, behind the fronts' checks of their own arguments: words the K frequency words, D and R per
// channel, taps[k] channel k's prototype or empty for the default design of taps_per_phase D_k taps, overlap < 0 for the
// default.  Messages speak of the arrays of gr4pm_fft_ddc_mixed_params; the FftDdc's front has refused every scalar they
// could name before it calls this.
gr4pm_status create_bank(FftDdcBank& h, const char* name, std::vector<uint32_t> words, const std::vector<size_t>& D,
                         const std::vector<size_t>& R, std::vector<std::vector<float>> taps, size_t taps_per_phase, ptrdiff_t overlap,
                         uint64_t start_index, void* stream)
{
    const size_t K = words.size();
    std::vector<size_t> L(K);
    for (size_t k = 0; k < K; ++k) {
        if (!fft_ddc_pow2(D[k]) || D[k] < kFftDdcMinD || D[k] > kFftDdcMaxD) {
            set_error("%s: decimations[%zu] must be a power of two in [%u, %u], not %zu", name, k, kFftDdcMinD, kFftDdcMaxD, D[k]);
            return GR4PM_ERR_INVALID;
        }
        if (taps[k].empty() && (taps_per_phase < 1 || taps_per_phase * D[k] > kN)) {
            set_error("%s: %zu taps per phase at a decimation of %zu: the prototype has 1 .. %zu taps", name, taps_per_phase, D[k], kN);
            return GR4PM_ERR_INVALID;
        }
        L[k] = taps[k].empty() ? taps_per_phase * D[k] : taps[k].size();
    }
    const FftDdcMixedVerdict sizes = fft_ddc_mixed_validate_channels(K, D.data(), R.data(), L.data());
    if (sizes.refusal == FftDdcMixedRefusal::images) {
        set_error("%s: images[%zu] must be a power of two in [1, %zu], not %zu", name, sizes.channel, D[sizes.channel], R[sizes.channel]);
        return GR4PM_ERR_INVALID;
    }
    if (sizes.refusal != FftDdcMixedRefusal::none) {
        set_error("%s: invalid sizes of channel %zu", name, sizes.channel);
        return GR4PM_ERR_INVALID;
    }
    for (size_t k = 0; k < K; ++k) {
        if (taps[k].empty()) {
            taps[k].resize(L[k]);
            GR4PM_TRY(gr4pm_ddc_taps(D[k], taps_per_phase, 0.25, 0.75, taps[k].data()));
        }
        for (size_t t = 0; t < L[k]; ++t)
            if (!std::isfinite(taps[k][t])) {
                set_error("%s: taps[%zu] of channel %zu is not finite", name, t, k);
                return GR4PM_ERR_INVALID;
            }
    }
    const size_t Dmax = fft_ddc_mixed_max_decimation(K, D.data());
    const size_t V = overlap < 0 ? fft_ddc_mixed_default_overlap(K, D.data(), L.data()) : static_cast<size_t>(overlap);
    const FftDdcMixedVerdict v = fft_ddc_mixed_validate(K, D.data(), R.data(), L.data(), V);
    switch (v.refusal) {
    case FftDdcMixedRefusal::none: break;
    case FftDdcMixedRefusal::overlap_multiple:
        set_error("%s: the overlap %zu is no multiple of the largest decimation %zu", name, V, Dmax);
        return GR4PM_ERR_INVALID;
    case FftDdcMixedRefusal::overlap_low:
        set_error("%s: the overlap %zu is below the reach of channel %zu: %zu taps at a decimation of %zu beside %zu need %zu", name, V,
                  v.channel, L[v.channel], D[v.channel], Dmax, Dmax - D[v.channel] + L[v.channel] - 1);
        return GR4PM_ERR_INVALID;
    case FftDdcMixedRefusal::overlap_high:
        set_error("%s: the overlap %zu leaves a hop below %u: at most %zu", name, V, kFftDdcMinHop, kN - kFftDdcMinHop);
        return GR4PM_ERR_INVALID;
    default: set_error("%s: invalid sizes", name); return GR4PM_ERR_INVALID;
    }
    GR4PM_TRY(require_device());
    h.name = name, h.K = K, h.V = V;
    h.words = std::move(words);
    h.start_index = start_index;
    h.shape = fft_ddc_shape(static_cast<uint32_t>(Dmax), static_cast<uint32_t>(V));
    h.stream = static_cast<hipStream_t>(stream);
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
        h.max_waves = std::min(h.max_waves, static_cast<size_t>(prop.multiProcessorCount) * kW64Waves);
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
    std::vector<size_t> offsets(K);
    std::vector<float2> G(fft_ddc_mixed_table_offsets(K, D.data(), R.data(), offsets.data()));
    std::vector<MixedDesc> desc(K);
    h.channels.resize(K);
    for (size_t k = 0; k < K; ++k) {
        const uint32_t w = h.words[k], c = fft_ddc_bin(w);
        const size_t RB = R[k] * (kN / D[k]);
        for (size_t t = 0; t < RB; ++t)
            G[offsets[k] + t] = response(taps[k], w, c, static_cast<int32_t>(t) - static_cast<int32_t>(RB / 2));
        h.channels[k] = fft_ddc_mixed_channel(static_cast<uint32_t>(Dmax), static_cast<uint32_t>(V), static_cast<uint32_t>(D[k]));
        h.max_frames = std::max(h.max_frames, h.channels[k].frames);
        desc[k] = MixedDesc{w, static_cast<uint32_t>(__builtin_ctzll(kN / D[k])), static_cast<uint32_t>(R[k]), h.channels[k].first,
                            static_cast<uint32_t>(D[k]), h.channels[k].frames, static_cast<uint32_t>(offsets[k]), static_cast<uint32_t>(k)};
    }
    if (std::all_of(desc.begin(), desc.end(), [&](const MixedDesc& d) { return d.D == desc[0].D && d.R == desc[0].R; })) h.alike = desc[0];
    // the longest inverse transforms first: a workgroup at B = 512 costs many times one at B = 32
    std::stable_sort(desc.begin(), desc.end(), [](const MixedDesc& x, const MixedDesc& y) { return x.logB > y.logB; });
    GR4PM_TRY(h.d_tT.alloc(tT.size()));
    GR4PM_TRY(h.d_cc.alloc(cc.size()));
    GR4PM_TRY(h.d_tw.alloc(tw.size()));
    GR4PM_TRY(h.d_spec.alloc(kChunk * kN));
    GR4PM_TRY(h.tail.alloc(0, kN, 1, h.stream));
    GR4PM_TRY(h.d_G.alloc(G.size()));
    GR4PM_TRY(h.d_desc.alloc(K));
    GR4PM_TRY(h.d_w.alloc(K));
    GR4PM_TRY(h.d_tT.upload(tT.data(), tT.size(), h.stream));
    GR4PM_TRY(h.d_cc.upload(cc.data(), cc.size(), h.stream));
    GR4PM_TRY(h.d_tw.upload(tw.data(), tw.size(), h.stream));
    GR4PM_TRY(h.d_G.upload(G.data(), G.size(), h.stream));
    GR4PM_TRY(h.d_desc.upload(desc.data(), K, h.stream));
    GR4PM_TRY(h.d_w.upload(h.words.data(), K, h.stream));
    GR4PM_HIP_TRY(hipStreamSynchronize(h.stream)); // the uploads read this function's vectors
    return GR4PM_OK;
}

gr4pm_status check_samples(const FftDdcBank& h, size_t n_in)
{
    if (n_in > (size_t(1) << 40)) {
        set_error("%s: %zu samples in one call, at most 2^40", h.name, n_in);
        return GR4PM_ERR_OVERFLOW;
    }
    return GR4PM_OK;
}

// frames per row of a call: counts[k]
void frames_of(const FftDdcBank& h, const FftDdcPlan& p, size_t* counts)
{
    for (size_t k = 0; k < h.K; ++k) counts[k] = fft_ddc_mixed_frames(p, h.channels[k]);
}

// The call of both handles: per launch pair of at most kChunk segments the forward kernel, then the channel kernel; then
// the tail.  format iq::kC64 for complex64 samples; counts[K]
gr4pm_status process_any(FftDdcBank& h, const void* in, int format, float scale, size_t n_in, gr4pm_c64* out, size_t out_stride,
                         size_t out_cap_frames, size_t* counts)
{
    std::fill(counts, counts + h.K, size_t(0));
    GR4PM_TRY(check_samples(h, n_in));
    if (n_in == 0) return GR4PM_OK;
    if (!in) {
        set_error("%s: no input array", h.name);
        return GR4PM_ERR_INVALID;
    }
    const FftDdcPlan p = fft_ddc_plan(h.shape, h.taken, n_in);
    const size_t longest = p.n_segments * h.max_frames;
    if (longest > out_cap_frames) {
        set_error("%s: %zu frames a row, room for %zu", h.name, longest, out_cap_frames);
        return GR4PM_ERR_OVERFLOW;
    }
    if (longest && (!out || (h.K > 1 && out_stride < longest))) {
        set_error("%s: no output array, or a row stride of %zu items for %zu frames", h.name, out_stride, longest);
        return GR4PM_ERR_INVALID;
    }
    // the samples in front of the virtual stream (V = 0 only) belong to no frame
    const size_t item = format == iq::kC64 ? sizeof(float2) : iq::item_bytes(format);
    const void* x = static_cast<const char*>(in) + p.drop * item;
    const StreamTail::Plan t = {h.tail.d_hist[h.tail.cur].p, h.tail.d_hist[1 - h.tail.cur].p, p.tail, p.n_segments, p.tail_new, p.tail_new};
    FwdArgs a = {};
    a.hist = t.hist, a.in = x, a.H = p.tail;
    a.tT = h.d_tT.p, a.cc = h.d_cc.p, a.spec = h.d_spec.p;
    a.hop = h.shape.hop, a.scale = scale;
    MixedArgs b = {};
    b.spec = reinterpret_cast<const float2*>(h.d_spec.p), b.G = h.d_G.p, b.tw = h.d_tw.p, b.desc = h.d_desc.p;
    b.out = reinterpret_cast<float2*>(out), b.out_stride = out_stride;
    b.call_segments = p.n_segments, b.hop = h.shape.hop, b.max_frames = h.max_frames;
    ChanArgs c = {};
    c.spec = b.spec, c.G = b.G, c.tw = b.tw, c.w = h.d_w.p, c.out = b.out, c.out_stride = out_stride;
    c.D = h.alike.D, c.logB = h.alike.logB, c.R = h.alike.R, c.first = h.alike.first, c.hop = h.shape.hop;
    iq::with_format(format, [&](auto f) {
        for (size_t done = 0; done < p.n_segments;) {
            const size_t segs = std::min(p.n_segments - done, kChunk);
            const size_t per_wave = (segs + h.max_waves - 1) / h.max_waves;
            const size_t waves = (segs + per_wave - 1) / per_wave;
            a.seg0 = done, a.n_seg = static_cast<uint32_t>(segs), a.run = static_cast<uint32_t>(per_wave);
            hipLaunchKernelGGL(k_fft_ddc_forward<decltype(f)::value>, dim3(static_cast<unsigned>((waves + kW64Waves - 1) / kW64Waves)),
                               dim3(kW64Threads), 0, h.stream, a);
            const dim3 grid(static_cast<unsigned>(segs), static_cast<unsigned>(h.K));
            b.seg0 = done, c.frame0 = done * h.alike.frames;
            b.index0 = c.index0 = fft_ddc_segment_index(h.shape, h.start_index, p.segments_before + done);
            if (h.alike.logB)
                hipLaunchKernelGGL(k_fft_ddc_channel, grid, dim3(64), 0, h.stream, c);
            else
                hipLaunchKernelGGL(k_fft_ddc_mixed, grid, dim3(64), 0, h.stream, b);
            done += segs;
        }
        h.tail.launch_history<decltype(f)::value>(t, x, 0, p.n_used, scale, h.stream);
    });
    GR4PM_HIP_TRY(hipGetLastError());
    h.tail.commit(t);
    h.taken += n_in;
    frames_of(h, p, counts);
    return GR4PM_OK;
}

// process_iq() of both handles
gr4pm_status process_iq(FftDdcBank& h, const void* in, int format, float scale, size_t n_in, gr4pm_c64* out, size_t out_stride,
                        size_t out_cap_frames, size_t* counts)
{
    std::fill(counts, counts + h.K, size_t(0));
    if (!iq::valid(format)) {
        set_error("%s: format %d is none of GR4PM_IQ_SC16 / SC8 / CU8", h.name, format);
        return GR4PM_ERR_INVALID;
    }
    return process_any(h, in, format, scale == 0.0f ? iq::default_scale(format) : scale, n_in, out, out_stride, out_cap_frames, counts);
}

gr4pm_status frames_for(const FftDdcBank& h, size_t n_in, size_t* counts)
{
    std::fill(counts, counts + h.K, size_t(0));
    GR4PM_TRY(check_samples(h, n_in));
    frames_of(h, fft_ddc_plan(h.shape, h.taken, n_in), counts);
    return GR4PM_OK;
}

void destroy(FftDdcBank* h)
{
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    delete h;
}

gr4pm_status reset(FftDdcBank* h)
{
    if (!h) return GR4PM_ERR_INVALID;
    GR4PM_TRY(h->tail.reset(h->stream));
    h->taken = 0;
    return GR4PM_OK;
}

gr4pm_status frequencies(const FftDdcBank* h, double* out)
{
    if (!h || !out) return GR4PM_ERR_INVALID;
    for (size_t k = 0; k < h->K; ++k) out[k] = folded_frequency(h->words[k]);
    return GR4PM_OK;
}

gr4pm_status sizes(const FftDdcBank* h, size_t* overlap, size_t* hop)
{
    if (!h || !overlap || !hop) return GR4PM_ERR_INVALID;
    *overlap = h->V;
    *hop = h->shape.hop;
    return GR4PM_OK;
}

} // namespace

// distinct types for the ABI, one bank behind both
struct gr4pm_fft_ddc : FftDdcBank {};
struct gr4pm_fft_ddc_mixed : FftDdcBank {};

extern "C" {

gr4pm_status gr4pm_fft_ddc_taps(size_t decimation, size_t taps_per_phase, float* out)
try {
    if (!out) return GR4PM_ERR_INVALID;
    GR4PM_TRY(check_decimation(decimation));
    return gr4pm_ddc_taps(decimation, taps_per_phase, 0.25, 0.75, out);
}
GR4PM_ABI_CATCH

// the bank of K equal channels, behind the checks that name this entry's own scalars
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
    if (!p->taps && (p->taps_per_phase < 1 || p->taps_per_phase * D > kN)) {
        set_error("fft_ddc: %zu taps per phase at a decimation of %zu: the prototype has 1 .. %zu taps", p->taps_per_phase, D, kN);
        return GR4PM_ERR_INVALID;
    }
    const size_t L = p->taps ? p->n_taps : p->taps_per_phase * D;
    for (size_t t = 0; p->taps && t < L; ++t)
        if (!std::isfinite(p->taps[t])) {
            set_error("fft_ddc: taps[%zu] is not finite", t);
            return GR4PM_ERR_INVALID;
        }
    if (p->overlap >= 0) { // the default is a multiple of 256 that reaches; at most it is too high, which the bank says
        const size_t V = static_cast<size_t>(p->overlap);
        if (V % D) {
            set_error("fft_ddc: the overlap %zu is no multiple of the decimation %zu", V, D);
            return GR4PM_ERR_INVALID;
        }
        if (V <= kN - kFftDdcMinHop && V + 1 < L) {
            set_error("fft_ddc: the overlap %zu is below the %zu taps' reach of %zu samples", V, L, L - 1);
            return GR4PM_ERR_INVALID;
        }
    }
    std::unique_ptr<gr4pm_fft_ddc> h(new (std::nothrow) gr4pm_fft_ddc);
    if (!h) return GR4PM_ERR_NOMEM;
    const std::vector<float> taps = p->taps ? std::vector<float>(p->taps, p->taps + L) : std::vector<float>();
    GR4PM_TRY(create_bank(*h, "fft_ddc", std::move(words), std::vector<size_t>(K, D), std::vector<size_t>(K, R),
                          std::vector<std::vector<float>>(K, taps), p->taps_per_phase, p->overlap, p->start_index, p->stream));
    *out = h.release();
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

void gr4pm_fft_ddc_destroy(gr4pm_fft_ddc* h)
try {
    destroy(h);
}
GR4PM_ABI_CATCH_VOID

gr4pm_status gr4pm_fft_ddc_reset(gr4pm_fft_ddc* h)
try {
    return reset(h);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_ddc_frames_for(const gr4pm_fft_ddc* h, size_t n_in, size_t* n_frames)
try {
    if (!h || !n_frames) return GR4PM_ERR_INVALID;
    size_t counts[kFftDdcMaxK];
    const gr4pm_status st = frames_for(*h, n_in, counts);
    *n_frames = counts[0]; // every row's
    return st;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_ddc_frequencies(const gr4pm_fft_ddc* h, double* out)
try {
    return frequencies(h, out);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_ddc_sizes(const gr4pm_fft_ddc* h, size_t* overlap, size_t* hop)
try {
    return sizes(h, overlap, hop);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_ddc_process(gr4pm_fft_ddc* h, const gr4pm_c64* in, size_t n_in, gr4pm_c64* out, size_t out_stride,
                                   size_t out_cap_frames, size_t* n_frames)
try {
    if (!h || !n_frames) return GR4PM_ERR_INVALID;
    size_t counts[kFftDdcMaxK];
    const gr4pm_status st = process_any(*h, in, iq::kC64, 0.0f, n_in, out, out_stride, out_cap_frames, counts);
    *n_frames = counts[0];
    return st;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_ddc_process_iq(gr4pm_fft_ddc* h, const void* in, int format, float scale, size_t n_in, gr4pm_c64* out,
                                      size_t out_stride, size_t out_cap_frames, size_t* n_frames)
try {
    if (n_frames) *n_frames = 0;
    if (!h || !n_frames) return GR4PM_ERR_INVALID;
    size_t counts[kFftDdcMaxK];
    const gr4pm_status st = process_iq(*h, in, format, scale, n_in, out, out_stride, out_cap_frames, counts);
    *n_frames = counts[0];
    return st;
}
GR4PM_ABI_CATCH

// ---- MixedFftDdc: a decimation per channel ---------------------------------------------------------

gr4pm_status gr4pm_fft_ddc_mixed_create(const gr4pm_fft_ddc_mixed_params* p, gr4pm_fft_ddc_mixed** out)
try {
    if (!p || !out) return GR4PM_ERR_INVALID;
    *out = nullptr;
    const size_t K = p->n_channels;
    std::vector<uint32_t> words;
    GR4PM_TRY(frequency_words("fft_ddc_mixed", p->frequencies, K, kFftDdcMaxK, words));
    if (!p->decimations) {
        set_error("fft_ddc_mixed: no decimations");
        return GR4PM_ERR_INVALID;
    }
    if ((p->taps == nullptr) != (p->n_taps == nullptr)) {
        set_error("fft_ddc_mixed: taps and n_taps come together or not at all");
        return GR4PM_ERR_INVALID;
    }
    std::vector<std::vector<float>> taps(K);
    for (size_t k = 0, at = 0; p->taps && k < K; at += p->n_taps[k], ++k) {
        GR4PM_TRY(prototype_length("fft_ddc_mixed", p->taps, p->n_taps[k], kN));
        taps[k].assign(p->taps + at, p->taps + at + p->n_taps[k]);
    }
    std::unique_ptr<gr4pm_fft_ddc_mixed> h(new (std::nothrow) gr4pm_fft_ddc_mixed);
    if (!h) return GR4PM_ERR_NOMEM;
    GR4PM_TRY(create_bank(*h, "fft_ddc_mixed", std::move(words), std::vector<size_t>(p->decimations, p->decimations + K),
                          p->images ? std::vector<size_t>(p->images, p->images + K) : std::vector<size_t>(K, 2), std::move(taps),
                          p->taps_per_phase, p->overlap, p->start_index, p->stream));
    *out = h.release();
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

void gr4pm_fft_ddc_mixed_destroy(gr4pm_fft_ddc_mixed* h)
try {
    destroy(h);
}
GR4PM_ABI_CATCH_VOID

gr4pm_status gr4pm_fft_ddc_mixed_reset(gr4pm_fft_ddc_mixed* h)
try {
    return reset(h);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_ddc_mixed_frames_for(const gr4pm_fft_ddc_mixed* h, size_t n_in, size_t* n_frames)
try {
    if (!h || !n_frames) return GR4PM_ERR_INVALID;
    return frames_for(*h, n_in, n_frames);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_ddc_mixed_frequencies(const gr4pm_fft_ddc_mixed* h, double* out)
try {
    return frequencies(h, out);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_ddc_mixed_sizes(const gr4pm_fft_ddc_mixed* h, size_t* overlap, size_t* hop)
try {
    return sizes(h, overlap, hop);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_ddc_mixed_process(gr4pm_fft_ddc_mixed* h, const gr4pm_c64* in, size_t n_in, gr4pm_c64* out, size_t out_stride,
                                         size_t out_cap_frames, size_t* n_frames)
try {
    if (!h || !n_frames) return GR4PM_ERR_INVALID;
    return process_any(*h, in, iq::kC64, 0.0f, n_in, out, out_stride, out_cap_frames, n_frames);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_ddc_mixed_process_iq(gr4pm_fft_ddc_mixed* h, const void* in, int format, float scale, size_t n_in,
                                            gr4pm_c64* out, size_t out_stride, size_t out_cap_frames, size_t* n_frames)
try {
    if (!h || !n_frames) return GR4PM_ERR_INVALID;
    return process_iq(*h, in, format, scale, n_in, out, out_stride, out_cap_frames, n_frames);
}
GR4PM_ABI_CATCH

} // extern "C"
