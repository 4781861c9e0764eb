// ddc.hip -- tunable down-converter: K frequency-translating decimating FIRs over one wideband c64 stream, any integer
// decimation D, channel-major output (out[k][n], the layout gr4pm_multichannel_receiver_submit takes).  The project's
// own block (the reference is a one-channel modem).  Definition (include/gr4pm_hip.h):
//     w_k = llrint(f_k 2^32) mod 2^32,   phi_k(i) = (w_k i) mod 2^32  (wrapping unsigned arithmetic, exact anywhere)
//     y_k[n] = sum_t h[t] x[i - t] exp(-2 pi j phi_k(i - t) / 2^32),   i = start_index + n D + D - 1,   x = 0 before the start
// evaluated in the rotated-taps form
//     g_k[t] = h[t] exp(+2 pi j phi_k(t) / 2^32)     (host, double, rounded to float once, a K x L table on the device)
//     r_k[n] = exp(-2 pi j phi_k(i) / 2^32)          (device, double sincospi of -phi / 2^31, rounded to float)
//     y_k[n] = r_k[n] sum_t g_k[t] x[i - t]          (one accumulator per channel, t ascending, four fmaf per product)
//
// k_ddc: a workgroup owns T consecutive frames (T <= 256: a lane owns one frame) and up to 8 channels (blockIdx.y).
//   The (T - 1) D + Lc samples the tile needs for Lc taps go to LDS once, converted on the way in and laid out by
//   phase: sample j of the stage at row j mod D, column j div D, rows of an odd number of items.  Lanes on consecutive
//   frames then read consecutive items of one row for every tap (no stride-D bank conflicts), and the 16 consecutive
//   samples of a staging store fall on 16 different rows, so on different banks.  One LDS read of a sample feeds the
//   group's complex MACs in registers; g_k[t] is the same address in every lane, and the table holds a group's taps
//   interleaved by channel, so the taps of one t sit side by side.  The host picks T and Lc so that the stage stays
//   within 64 KiB: L > Lc runs the t loop over re-staged chunks, still ascending in t, so chunking changes no bit.  Each channel's T items leave as one contiguous run, lanes on consecutive items.
//   One form serves every size: a tile shrinks to T >= 3 frames at D = 1024, which wastes lanes but not correctness.
// Every result is a function of (channel, frame, stream) only: it does not depend on how the stream is cut into calls.
// The stream's tail -- the last L - 1 samples plus the incomplete frame -- is stream_tail.hpp's: its kernel moves it to
// the handle's other history buffer.  The tile's sizes are hostlogic/xlate_geometry.hpp's ddc_geometry(): the handle
// keeps them in a prefilled DdcArgs, and a call writes only what changes from call to call.
// Integer input (gr4pm_ddc_process_iq): both kernels are templated on the input format and convert where a sample
// enters them with iq_format.hpp's unpack_item(), the very expression gr4pm_iq_unpack evaluates; the stage and the
// history stay complex64, so the result is that of process() on the unpacked samples bit for bit.
//
// Rational resampling by I / D (gr4pm_ddc_create_rational): output item n of the handle has the
// upsampled index m = n D + D - 1, the input index i = start_index + m div I and the polyphase branch p = m mod I:
//     y_k[n] = r_k[n] sum_s g_k[p][s] x[i - s],   g_k[p][s] = h[p + s I] exp(+2 pi j phi_k(s) / 2^32),   s ascending
// With gcd(I, D) = 1 the items of branch p are I apart and their input indices D apart: every branch is an integer-D
// Ddc with the taps h[p::I], evaluated by the very loop of ddc_tile.
// k_ddc_rational: a workgroup owns I T consecutive items (T <= 64 per branch) and up to 8 channels.  The input span of
//   the tile, about T D + P samples, goes to LDS once in ddc_tile's layout and serves all I branches.  A wave takes a
//   branch at a time (p = wave, wave + waves, ...: the taps of a wave are uniform), its lanes the branch's items; the
//   results pass through a second LDS region as [channel][item of the tile], so that every channel's I T items leave
//   as one contiguous run.  The host picks T so that both regions stay within 64 KiB; the taps are never chunked.
//   I = 1 does not come here: such a handle runs k_ddc.  The tile is rddc_geometry()'s, the position in the stream
//   hostlogic/resample_position.hpp's with lead = D - 1: 64-bit integers on the host, by value to the kernel.
// Both creates are one create(): gr4pm_ddc_create's is the ratio 1 / D.
//
// Burst spans of a recording (gr4pm_ddc_extract): since a result is a function of (channel, frame,
// stream) only, k_ddc_extract computes up to 64 (channel, first frame, frame count) spans of an integer-D handle's output on
// their own, each into a zero-padded row, with ddc_tile's stage and loop for one channel: the bits of the stream's slices.
// The stream state is not touched; hostlogic/extract_plan.hpp validates the call and states the kernel's indices.
#include "freq_xlate.hpp"
#include "hostlogic/extract_plan.hpp"
#include "hostlogic/resample_position.hpp"
#include "kaiser_design.hpp"
#include "stream_tail.hpp"

#include <cmath>

namespace {

namespace iq = gr4pm::iq;
using namespace gr4pm::hostlogic;
using gr4pm::cmac;
using gr4pm::ConstTaps;

constexpr size_t kMaxK = 64, kMaxI = 64, kMaxD = 1024, kMaxL = 8192;

struct DdcArgs {
    const float2* hist;   // the H samples in front of in[0]: L - 1 of history, then the carried partial frame
    const void* in;       // complex64, or items of the kernel's integer format
    float2* out;
    const float2* g;      // rotated taps, K L items: group by group, a group's as [L][its channels]
    const uint32_t* w;    // [K] frequency words
    size_t H;
    size_t total;         // H + n_in: samples of the virtual stream hist ++ in
    size_t out_stride;
    size_t n_frames;
    uint64_t pos;         // absolute index of the virtual stream's sample L - 1 (the first one not yet in a frame)
    unsigned K, D, L;
    DdcTile tile;
    float scale;          // of an integer format's unpack
};

// NC: channels of this workgroup's group; F: the input's format (iq::kC64: complex64)
template <int NC, int F>
__device__ __forceinline__ void ddc_tile(const DdcArgs& a, float2* s)
{
    const unsigned tid = threadIdx.x;
    const unsigned D = a.D, L = a.L, T = a.tile.T, RS = a.tile.RS;
    const size_t f0 = static_cast<size_t>(blockIdx.x) * T;
    const unsigned k0 = blockIdx.y * kGroup;
    const float2* __restrict__ g = a.g + static_cast<size_t>(k0) * L;

    float2 acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = float2{0.0f, 0.0f};

    for (unsigned t0 = 0; t0 < L; t0 += a.tile.Lc) {
        const unsigned lc = L - t0 < a.tile.Lc ? L - t0 : a.tile.Lc;
        // stage item j: virtual sample vb + j; frame f0 + n takes tap t from item n D + (t0 + lc - 1 - t)
        const size_t vb = static_cast<size_t>(L - 1) + f0 * D + (D - 1) - (t0 + lc - 1);
        if (t0) __syncthreads(); // the previous chunk has been read
        gr4pm::stage_by_phase(s, (T - 1) * D + lc, kNt, D, a.tile.rcpD, RS, vb, a.total,
                              [&](size_t v) { return iq::vsample<F>(a.hist, a.H, a.in, a.scale, v); });
        __syncthreads();
        if (tid < T) {
            unsigned t = t0;
            unsigned col = (lc - 1) / D, row = (lc - 1) - col * D;
            for (;;) {
                const float2* sp = s + row * RS + col + tid;
#pragma unroll 4
                for (unsigned r = 0; r <= row; ++r, sp -= RS, ++t) {
                    const float2 x = *sp;
#pragma unroll
                    for (int c = 0; c < NC; ++c) cmac(acc[c], g[t * NC + c], x);
                }
                if (col == 0) break;
                --col;
                row = D - 1;
            }
        }
    }

    const size_t f = f0 + tid;
    if (tid < T && f < a.n_frames) {
        const uint32_t i = static_cast<uint32_t>(a.pos + f * D + (D - 1)); // the low 32 bits are all the phase needs
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            float2 y = {0.0f, 0.0f};
            cmac(y, gr4pm::mixer<-1>(a.w[k0 + c], i), acc[c]);
            a.out[static_cast<size_t>(k0 + c) * a.out_stride + f] = y;
        }
    }
}

template <int F>
__global__ __launch_bounds__(kNt) void k_ddc(DdcArgs a)
{
    extern __shared__ float2 s_ddc[];
    gr4pm::with_channels(a.K - blockIdx.y * kGroup, [&](auto nc) { ddc_tile<decltype(nc)::value, F>(a, s_ddc); });
}

struct ExtractArgs {
    const void* in;       // the buffer's first sample at or after the handle's start: item 0 is the kernel's index lo
    float2* out;          // [spans][out_stride]
    const float2* g;      // the handle's rotated taps
    const uint32_t* w;    // [K] frequency words
    uint64_t lo, hi;      // the buffer in the kernel's indices (hostlogic/extract_plan.hpp); zero outside
    uint64_t start;       // the handle's start_index
    size_t out_stride;
    size_t n_cols;
    unsigned K, D, L;
    DdcTile tile;
    float scale;
    ExtractSpan spans[kMaxExtractSpans];
};

// blockIdx.y: the span, blockIdx.x: a tile of T columns of its row; one channel per workgroup, so the span, the
// channel and the tile's first frame are wave-uniform.  ddc_tile's stage and loop with NC = 1 over the channel's
// column of its group's interleaved table, restated because the tile here is made of a span's frames.
template <int F>
__global__ __launch_bounds__(kNt) void k_ddc_extract(ExtractArgs a)
{
    extern __shared__ float2 s_ext[];
    float2* s = s_ext;
    const unsigned tid = threadIdx.x;
    const unsigned D = a.D, L = a.L, T = a.tile.T, RS = a.tile.RS;
    const ExtractSpan span = a.spans[blockIdx.y];
    const uint64_t c0 = static_cast<uint64_t>(blockIdx.x) * T; // the tile's first column
    const unsigned nv = extract_tile_frames(c0, span.n_frames, T);
    float2* __restrict__ row = a.out + static_cast<size_t>(blockIdx.y) * a.out_stride;
    if (nv == 0) { // wholly at or behind the span's end
        if (tid < T && c0 + tid < a.n_cols) row[c0 + tid] = float2{0.0f, 0.0f};
        return;
    }
    const unsigned k = span.channel, k0 = k / kGroup * kGroup;
    const unsigned nc = a.K - k0 < static_cast<unsigned>(kGroup) ? a.K - k0 : static_cast<unsigned>(kGroup);
    const float2* __restrict__ g = a.g + static_cast<size_t>(k0) * L + (k - k0); // tap t: g[t nc]
    const uint64_t f0 = span.first_frame + c0;

    float2 acc = {0.0f, 0.0f};
    for (unsigned t0 = 0; t0 < L; t0 += a.tile.Lc) {
        const unsigned lc = L - t0 < a.tile.Lc ? L - t0 : a.tile.Lc;
        // stage item j: sample vb + j; frame f0 + n takes tap t from item n D + (t0 + lc - 1 - t)
        const uint64_t vb = extract_stage_base(L, D, f0, t0, lc);
        if (t0) __syncthreads(); // the previous chunk has been read
        gr4pm::stage_by_phase(s, static_cast<unsigned>(extract_stage_items(D, nv, lc)), kNt, D, a.tile.rcpD, RS, vb, a.hi,
                              [&](size_t u) {
                                  if (u < a.lo) return float2{0.0f, 0.0f};
                                  if constexpr (F == iq::kC64)
                                      return static_cast<const float2*>(a.in)[u - a.lo];
                                  else
                                      return iq::unpack_item<F>(iq::load_item<F>(a.in, u - a.lo), a.scale);
                              });
        __syncthreads();
        if (tid < nv) {
            unsigned t = t0;
            unsigned col = (lc - 1) / D, r0 = (lc - 1) - col * D;
            for (;;) {
                const float2* sp = s + r0 * RS + col + tid;
#pragma unroll 4
                for (unsigned r = 0; r <= r0; ++r, sp -= RS, ++t) cmac(acc, g[static_cast<size_t>(t) * nc], *sp);
                if (col == 0) break;
                --col;
                r0 = D - 1;
            }
        }
    }

    if (tid < T && c0 + tid < a.n_cols) {
        float2 y = {0.0f, 0.0f};
        if (tid < nv) {
            const uint32_t i = static_cast<uint32_t>(a.start + (f0 + tid) * D + (D - 1)); // the low 32 bits are all the phase needs
            cmac(y, gr4pm::mixer<-1>(a.w[k], i), acc);
        }
        row[c0 + tid] = y;
    }
}

struct RddcArgs {
    const float2* hist;   // the P - 1 samples in front of in[0]
    const void* in;       // complex64, or items of the kernel's integer format
    float2* out;
    const float2* g;      // rotated taps, K I P items: group by group, a group's as [I][P][its channels]
    const uint32_t* w;    // [K] frequency words
    size_t H;             // P - 1
    size_t total;         // H + n_in
    size_t out_stride;
    size_t n_frames;
    uint64_t pos;         // absolute index of in[0]
    uint64_t m0;          // the call's first item: its upsampled index, counted from in[0]'s
    unsigned K, D, I, L;
    unsigned P;           // ceil(L / I)
    RddcTile tile;
    float scale;
};

template <int NC, int F>
__device__ __forceinline__ void rddc_tile(const RddcArgs& a, float2* s)
{
    const unsigned tid = threadIdx.x, lane = tid & (kWave - 1);
    const unsigned wave = __builtin_amdgcn_readfirstlane(tid / kWave), waves = blockDim.x / kWave;
    const unsigned D = a.D, I = a.I, L = a.L, P = a.P, T = a.tile.T, RS = a.tile.RS;
    const unsigned IT = I * T;
    const size_t n0 = static_cast<size_t>(blockIdx.x) * IT; // the tile's first item
    const unsigned k0 = blockIdx.y * kGroup;
    const uint64_t m0 = a.m0 + static_cast<uint64_t>(n0) * D;
    const uint64_t c0 = m0 / I;                              // its sample, counted from in[0]
    const unsigned b0 = static_cast<unsigned>(m0 - c0 * I); // its branch
    // stage item j: virtual sample c0 + j, that is sample c0 - (P - 1) + j of the call; the tile's last item takes
    // its tap 0 from item (b0 + (I T - 1) D) div I + P - 1 < S
    gr4pm::stage_by_phase(s, ((IT - 1) * D + I - 1) / I + P, blockDim.x, D, a.tile.rcpD, RS, static_cast<size_t>(c0), a.total,
                          [&](size_t v) { return iq::vsample<F>(a.hist, a.H, a.in, a.scale, v); });
    __syncthreads();
    float2* so = s + RS * D; // [NC][I T]: the tile's results
    for (unsigned p = wave; p < I; p += waves) {
        // the branch's first item of the tile is item q: (b0 + q D) mod I = p; its lanes' items are q + I lane, their
        // samples D apart
        const unsigned q = (p + I - b0) % I * a.tile.Dinv % I;
        const unsigned e = (b0 + q * D) / I;           // its sample, counted from c0
        const unsigned Pp = p < L ? (L - p + I - 1) / I : 0; // taps of h[p::I]
        const size_t n = n0 + q + static_cast<size_t>(I) * lane;
        if (lane < T && n < a.n_frames) {
            const ConstTaps g = (ConstTaps)(a.g + (static_cast<size_t>(k0) * I + static_cast<size_t>(p) * NC) * P);
            float2 acc[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[c] = float2{0.0f, 0.0f};
            unsigned col = (e + P - 1) / D, row = (e + P - 1) - col * D, left = Pp, t = 0;
            while (left) {
                const unsigned run = row + 1 < left ? row + 1 : left;
                const float2* sp = s + row * RS + col + lane;
#pragma unroll 4
                for (unsigned r = 0; r < run; ++r, sp -= RS, ++t) {
                    const float2 x = *sp;
#pragma unroll
                    for (int c = 0; c < NC; ++c) cmac(acc[c], float2{g[2 * (t * NC + c)], g[2 * (t * NC + c) + 1]}, x);
                }
                left -= run;
                --col;
                row = D - 1;
            }
            const uint32_t i = static_cast<uint32_t>(a.pos + c0 + e + static_cast<uint64_t>(lane) * D); // the low 32 bits
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                float2 y = {0.0f, 0.0f};
                cmac(y, gr4pm::mixer<-1>(a.w[k0 + c], i), acc[c]);
                so[c * IT + q + I * lane] = y;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NC; ++c)
        for (unsigned ti = tid; ti < IT && n0 + ti < a.n_frames; ti += blockDim.x)
            a.out[static_cast<size_t>(k0 + c) * a.out_stride + n0 + ti] = so[c * IT + ti];
}

template <int F>
__global__ __launch_bounds__(kNt) void k_ddc_rational(RddcArgs a)
{
    extern __shared__ float2 s_rddc[];
    gr4pm::with_channels(a.K - blockIdx.y * kGroup, [&](auto nc) { rddc_tile<decltype(nc)::value, F>(a, s_rddc); });
}

// the two designs share their sizes' checks only; their band edges differ: the integer Ddc admits passband + stopband
// <= D of the output rate (band_edges_valid: a cutoff within fs / 2), the rational one at most min(1, D / I)
gr4pm_status design_taps(size_t D, size_t P, double passband, double stopband, std::vector<double>& h)
{
    GR4PM_TRY(gr4pm::design_sizes("ddc", 1, kMaxI, D, kMaxD, P, D, "a decimation", kMaxL));
    if (!gr4pm::band_edges_valid(passband, stopband, D, true)) {
        gr4pm::set_error("ddc: need 0 <= passband < stopband (units of the output rate) and a cutoff of at most fs / 2");
        return GR4PM_ERR_INVALID;
    }
    gr4pm::kaiser_lowpass(P * D, D, passband, stopband, h);
    return GR4PM_OK;
}

gr4pm_status design_rational_taps(size_t I, size_t D, size_t P, double passband, double stopband, std::vector<double>& h)
{
    GR4PM_TRY(gr4pm::design_sizes("ddc", I, kMaxI, D, kMaxD, P, D, "a decimation", kMaxL));
    // the cutoff, (passband + stopband) / 2 of the output rate fs I / D, within half of the output rate and half of fs
    const double most = D < I ? static_cast<double>(D) / static_cast<double>(I) : 1.0;
    if (!(passband >= 0.0 && passband < stopband && passband + stopband <= most)) {
        gr4pm::set_error("ddc: need 0 <= passband < stopband (units of the output rate fs %zu / %zu) and a cutoff of at most half of "
                         "the lower of the input and the output rate: passband + stopband <= %g", I, D, most);
        return GR4PM_ERR_INVALID;
    }
    gr4pm::kaiser_lowpass(P * D, D, passband, stopband, h, static_cast<double>(I));
    return GR4PM_OK;
}

} // namespace

struct gr4pm_ddc {
    size_t K = 0, D = 0, I = 1, max_frames = 0;
    uint64_t start_index = 0;
    gr4pm::StreamTail tail; // I = 1: L - 1 samples of history, then the incomplete frame; else P - 1 samples
    hipStream_t stream = nullptr;
    std::vector<uint32_t> words;
    gr4pm::DevBuf<float2> d_g;
    gr4pm::DevBuf<uint32_t> d_w;
    // what does not change from call to call, in the struct the handle's kernel takes
    DdcArgs args = {};  // I = 1; args.pos: absolute index of the first sample that is not yet part of a produced frame
    RddcArgs rargs = {}; // I > 1
    unsigned smem = 0, waves = 0; // of a launch
    gr4pm::hostlogic::ResamplePosition at; // I > 1: samples taken, the next item's sample and branch
};

using namespace gr4pm;

// process() and process_iq(): format iq::kC64 for complex64 samples
static gr4pm_status process_any(gr4pm_ddc* h, const void* in, int format, float scale, size_t n_in, gr4pm_c64* out,
                                size_t out_stride, size_t out_cap_frames, size_t* n_frames)
{
    if (!h || !n_frames) return GR4PM_ERR_INVALID;
    *n_frames = 0;
    const size_t D = h->D, I = h->I;
    if (n_in > (size_t(1) << 41) || n_in * I > h->max_frames * D) {
        set_error("ddc: %zu items at %zu / %zu, the handle was made for %zu output items a call", n_in, I, D, h->max_frames);
        return GR4PM_ERR_OVERFLOW;
    }
    if (n_in == 0) return GR4PM_OK;
    if (!in) {
        set_error("ddc: no input array");
        return GR4PM_ERR_INVALID;
    }
    const StreamTail::Plan t = h->tail.plan(n_in);
    const size_t F = I > 1 ? static_cast<size_t>(h->at.samples(n_in)) : t.n_frames;
    if (F > out_cap_frames) {
        set_error("ddc: %zu items, room for %zu", F, out_cap_frames);
        return GR4PM_ERR_OVERFLOW;
    }
    if (F && (!out || (h->K > 1 && out_stride < F))) {
        set_error("ddc: no output array, or a row stride of %zu items for %zu items", out_stride, F);
        return GR4PM_ERR_INVALID;
    }
    // a: a copy of the handle's prefilled argument struct, to which the call adds its own fields; kernel(format): the
    // instantiation to launch
    auto launch = [&](auto a, size_t tile, unsigned threads, auto kernel) {
        a.hist = t.hist;
        a.in = in;
        a.out = reinterpret_cast<float2*>(out);
        a.H = t.H;
        a.total = t.H + n_in;
        a.out_stride = out_stride;
        a.n_frames = F;
        a.scale = scale;
        const dim3 grid(static_cast<unsigned>((F + tile - 1) / tile), static_cast<unsigned>((h->K + kGroup - 1) / kGroup));
        iq::with_format(format, [&](auto f) {
            if (F) hipLaunchKernelGGL(kernel(f), grid, dim3(threads), h->smem, h->stream, a);
            h->tail.launch_history<decltype(f)::value>(t, in, 0, n_in, scale, h->stream);
        });
    };
    if (I > 1) {
        RddcArgs a = h->rargs;
        a.pos = h->start_index + h->at.taken;
        a.m0 = h->at.first();
        launch(a, I * a.tile.T, h->waves * kWave, [](auto f) { return &k_ddc_rational<decltype(f)::value>; });
    } else {
        launch(h->args, h->args.tile.T, kNt, [](auto f) { return &k_ddc<decltype(f)::value>; });
    }
    GR4PM_HIP_TRY(hipGetLastError());
    h->tail.commit(t);
    if (I > 1)
        h->at.advance(n_in, F);
    else
        h->args.pos += static_cast<uint64_t>(F) * D;
    *n_frames = F;
    return GR4PM_OK;
}

// extract() and extract_iq(): format iq::kC64 for complex64 samples.  hostlogic/extract_plan.hpp decides; the handle's
// stream state (tail, args.pos) is neither read nor written
static gr4pm_status extract_any(gr4pm_ddc* h, const void* in, int format, float scale, size_t n_in, uint64_t in_index,
                                const gr4pm_ddc_span* spans, size_t n_spans, gr4pm_c64* out, size_t out_stride, size_t n_cols)
{
    if (!h) return GR4PM_ERR_INVALID;
    const size_t L = h->I > 1 ? 1 : h->args.L;
    const ExtractPlan p = extract_plan(h->I, h->K, h->D, L, h->args.tile.T, h->start_index, in != nullptr, n_in, in_index,
                                       spans, n_spans, out != nullptr, out_stride, n_cols);
    switch (p.why) {
    case ExtractRefusal::none: break;
    case ExtractRefusal::nothing: return GR4PM_OK;
    case ExtractRefusal::rational:
        set_error("ddc: extract needs a handle with interpolation 1, this one resamples by %zu / %zu", h->I, h->D);
        return GR4PM_ERR_INVALID;
    case ExtractRefusal::spans:
        set_error("ddc: extract takes 1 .. %zu spans a call from a span array, not %zu", kMaxExtractSpans, n_spans);
        return GR4PM_ERR_INVALID;
    case ExtractRefusal::channel:
        set_error("ddc: spans[%zu].channel is %u, the handle has %zu channels", p.at, spans[p.at].channel, h->K);
        return GR4PM_ERR_INVALID;
    case ExtractRefusal::room:
        set_error("ddc: spans[%zu] has %u frames, a row has %zu columns", p.at, spans[p.at].n_frames, n_cols);
        return GR4PM_ERR_OVERFLOW;
    case ExtractRefusal::stride:
        set_error("ddc: a row stride of %zu items for %zu columns", out_stride, n_cols);
        return GR4PM_ERR_INVALID;
    case ExtractRefusal::overflow:
        if (p.at < n_spans)
            set_error("ddc: spans[%zu] (%u frames from frame %llu) reaches a sample index beyond 64 bits", p.at,
                      spans[p.at].n_frames, static_cast<unsigned long long>(spans[p.at].first_frame));
        else
            set_error("ddc: extract of %zu columns from %zu samples at index %llu does not fit the index range", n_cols, n_in,
                      static_cast<unsigned long long>(in_index));
        return GR4PM_ERR_OVERFLOW;
    case ExtractRefusal::input: set_error("ddc: no input array"); return GR4PM_ERR_INVALID;
    case ExtractRefusal::output: set_error("ddc: no output array"); return GR4PM_ERR_INVALID;
    }
    ExtractArgs a = {};
    const size_t item = format == iq::kC64 ? sizeof(float2) : iq::item_bytes(format);
    a.in = in ? static_cast<const char*>(in) + p.skip * item : nullptr;
    a.out = reinterpret_cast<float2*>(out);
    a.g = h->args.g, a.w = h->args.w;
    a.lo = p.lo, a.hi = p.hi;
    a.start = h->start_index;
    a.out_stride = out_stride;
    a.n_cols = n_cols;
    a.K = h->args.K, a.D = h->args.D, a.L = h->args.L;
    a.tile = h->args.tile;
    a.scale = scale;
    for (size_t b = 0; b < n_spans; ++b) a.spans[b] = spans[b];
    iq::with_format(format, [&](auto f) {
        hipLaunchKernelGGL(k_ddc_extract<decltype(f)::value>, dim3(p.grid_x, p.grid_y), dim3(kNt), h->smem, h->stream, a);
    });
    GR4PM_HIP_TRY(hipGetLastError());
    return GR4PM_OK;
}

// every format's instantiation of a kernel
#define GR4PM_DDC_ALL_FORMATS(kernel)                                                                                       \
    {reinterpret_cast<const void*>(&kernel<iq::kC64>), reinterpret_cast<const void*>(&kernel<GR4PM_IQ_SC16>),                \
     reinterpret_cast<const void*>(&kernel<GR4PM_IQ_SC8>), reinterpret_cast<const void*>(&kernel<GR4PM_IQ_CU8>)}

// both creates: gr4pm_ddc_create's handle is the ratio 1 / D
static gr4pm_status create(const gr4pm_ddc_rational_params* p, gr4pm_ddc** out)
{
    const size_t K = p->n_channels, D = p->decimation, I = p->interpolation;
    std::vector<uint32_t> words;
    GR4PM_TRY(frequency_words("ddc", p->frequencies, K, kMaxK, words));
    GR4PM_TRY(resample_ratio("ddc", I, kMaxI, D, kMaxD));
    GR4PM_TRY(per_call_cap("ddc", "max_frames", p->max_frames));
    GR4PM_TRY(prototype_length("ddc", p->taps, p->n_taps, kMaxL));
    std::vector<float> taps;
    GR4PM_TRY(taps_or_design(p->taps, p->n_taps, [&](std::vector<double>& hd) {
        return I > 1 ? design_rational_taps(I, D, 12, 0.25, 0.75, hd) : design_taps(D, 12, 0.25, 0.75, hd);
    }, taps));
    const size_t L = taps.size(), P = (L + I - 1) / I;
    GR4PM_TRY(require_device());
    std::unique_ptr<gr4pm_ddc> h(new (std::nothrow) gr4pm_ddc);
    if (!h) return GR4PM_ERR_NOMEM;
    h->K = K;
    h->D = D;
    h->I = I;
    h->max_frames = p->max_frames;
    h->start_index = p->start_index;
    h->stream = static_cast<hipStream_t>(p->stream);
    h->words = std::move(words);
    GR4PM_TRY(h->d_w.alloc(K));
    GR4PM_TRY(h->d_g.alloc(K * I * P));
    const unsigned Ku = static_cast<unsigned>(K), Du = static_cast<unsigned>(D), Lu = static_cast<unsigned>(L);
    if (I > 1) {
        RddcArgs& a = h->rargs;
        a.g = h->d_g.p, a.w = h->d_w.p;
        a.K = Ku, a.D = Du, a.I = static_cast<unsigned>(I), a.L = Lu, a.P = static_cast<unsigned>(P);
        RddcGeometry geo;
        if (!rddc_geometry(I, D, L, K, geo)) {
            set_error("ddc: no tile of %zu / %zu with %zu taps fits the stage", I, D, L);
            return GR4PM_ERR_INVALID;
        }
        a.tile = geo.tile, h->smem = geo.smem, h->waves = geo.waves;
        h->at.I = I, h->at.D = D, h->at.lead = D - 1;
        h->at.reset();
        if (h->smem > 48 * 1024)
            GR4PM_TRY(raise_dynamic_lds(GR4PM_DDC_ALL_FORMATS(k_ddc_rational), kDdcStageItems * sizeof(float2), "ddc"));
    } else {
        DdcArgs& a = h->args;
        a.g = h->d_g.p, a.w = h->d_w.p;
        a.pos = p->start_index;
        a.K = Ku, a.D = Du, a.L = Lu;
        const DdcGeometry geo = ddc_geometry(D, L);
        a.tile = geo.tile, h->smem = geo.smem;
        if (h->smem > 48 * 1024) {
            GR4PM_TRY(raise_dynamic_lds(GR4PM_DDC_ALL_FORMATS(k_ddc), kDdcStageItems * sizeof(float2), "ddc"));
            GR4PM_TRY(raise_dynamic_lds(GR4PM_DDC_ALL_FORMATS(k_ddc_extract), kDdcStageItems * sizeof(float2), "ddc"));
        }
    }
    // the rotated taps, a group's as [branch][s][channel]: tap s of a branch for all its channels side by side
    // (I = 1: one branch of L = P taps, tap t of all its channels side by side)
    std::vector<float2> g(K * I * P, float2{0.0f, 0.0f});
    for (size_t k = 0; k < K; ++k) {
        const uint32_t w = h->words[k];
        const size_t k0 = k / kGroup * kGroup, nc = K - k0 < static_cast<size_t>(kGroup) ? K - k0 : static_cast<size_t>(kGroup);
        for (size_t t = 0; t < L; ++t) {
            const size_t br = t % I, s = t / I;
            g[k0 * I * P + (br * P + s) * nc + (k - k0)] = rotated_tap(static_cast<double>(taps[t]), w * static_cast<uint32_t>(s));
        }
    }
    GR4PM_TRY(h->d_g.upload(g.data(), g.size(), h->stream));
    GR4PM_TRY(h->d_w.upload(h->words.data(), K, h->stream));
    GR4PM_TRY(h->tail.alloc(P - 1, I > 1 ? 1 : D, 1, h->stream));
    return finish_create(h, out, "ddc");
}

extern "C" {

gr4pm_status gr4pm_ddc_taps(size_t decimation, size_t taps_per_phase, double passband, double stopband, float* out)
try {
    if (!out) return GR4PM_ERR_INVALID;
    std::vector<double> h;
    GR4PM_TRY(design_taps(decimation, taps_per_phase, passband, stopband, h));
    round_taps(h, out);
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_ddc_create(const gr4pm_ddc_params* p, gr4pm_ddc** out)
try {
    if (!p || !out) return GR4PM_ERR_INVALID;
    *out = nullptr;
    const gr4pm_ddc_rational_params q = {p->n_channels, p->decimation, p->frequencies, p->taps, p->n_taps, p->max_frames,
                                         p->start_index, p->stream, 1};
    return create(&q, out);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_ddc_rational_taps(size_t interpolation, size_t decimation, size_t taps_per_phase, double passband,
                                     double stopband, float* out)
try {
    if (!out) return GR4PM_ERR_INVALID;
    std::vector<double> h;
    GR4PM_TRY(design_rational_taps(interpolation, decimation, taps_per_phase, passband, stopband, h));
    round_taps(h, out);
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_ddc_create_rational(const gr4pm_ddc_rational_params* p, gr4pm_ddc** out)
try {
    if (!p || !out) return GR4PM_ERR_INVALID;
    *out = nullptr;
    return create(p, out);
}
GR4PM_ABI_CATCH

void gr4pm_ddc_destroy(gr4pm_ddc* h)
try {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    delete h;
}
GR4PM_ABI_CATCH_VOID

gr4pm_status gr4pm_ddc_reset(gr4pm_ddc* h)
try {
    if (!h) return GR4PM_ERR_INVALID;
    GR4PM_TRY(h->tail.reset(h->stream));
    h->args.pos = h->start_index;
    h->at.reset();
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_ddc_output_items(const gr4pm_ddc* h, size_t n_in, size_t* n_frames)
try {
    if (!h || !n_frames) return GR4PM_ERR_INVALID;
    *n_frames = h->I > 1 ? static_cast<size_t>(h->at.samples(n_in)) : h->tail.frames(n_in);
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_ddc_frequencies(const gr4pm_ddc* h, double* out)
try {
    if (!h || !out) return GR4PM_ERR_INVALID;
    for (size_t k = 0; k < h->K; ++k) out[k] = folded_frequency(h->words[k]);
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_ddc_process(gr4pm_ddc* h, const gr4pm_c64* in, size_t n_in, gr4pm_c64* out, size_t out_stride,
                               size_t out_cap_frames, size_t* n_frames)
try {
    return process_any(h, in, iq::kC64, 0.0f, n_in, out, out_stride, out_cap_frames, n_frames);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_ddc_process_iq(gr4pm_ddc* h, const void* in, int format, float scale, size_t n_in, gr4pm_c64* out,
                                  size_t out_stride, size_t out_cap_frames, size_t* n_frames)
try {
    if (n_frames) *n_frames = 0;
    if (!iq::valid(format)) {
        set_error("ddc: format %d is none of GR4PM_IQ_SC16 / SC8 / CU8", format);
        return GR4PM_ERR_INVALID;
    }
    return process_any(h, in, format, scale == 0.0f ? iq::default_scale(format) : scale, n_in, out, out_stride, out_cap_frames,
                       n_frames);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_ddc_extract(gr4pm_ddc* h, const gr4pm_c64* in, size_t n_in, uint64_t in_index, const gr4pm_ddc_span* spans,
                               size_t n_spans, gr4pm_c64* out, size_t out_stride, size_t n_cols)
try {
    return extract_any(h, in, iq::kC64, 0.0f, n_in, in_index, spans, n_spans, out, out_stride, n_cols);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_ddc_extract_iq(gr4pm_ddc* h, const void* in, int format, float scale, size_t n_in, uint64_t in_index,
                                  const gr4pm_ddc_span* spans, size_t n_spans, gr4pm_c64* out, size_t out_stride,
                                  size_t n_cols)
try {
    if (!iq::valid(format)) {
        set_error("ddc: format %d is none of GR4PM_IQ_SC16 / SC8 / CU8", format);
        return GR4PM_ERR_INVALID;
    }
    return extract_any(h, in, format, scale == 0.0f ? iq::default_scale(format) : scale, n_in, in_index, spans, n_spans, out,
                       out_stride, n_cols);
}
GR4PM_ABI_CATCH

} // extern "C"
