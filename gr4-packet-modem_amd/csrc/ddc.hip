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
// the handle's other history buffer.
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
//   I = 1 does not come here: such a handle is gr4pm_ddc_create's.
#include "freq_xlate.hpp"
#include "kaiser_design.hpp"
#include "stream_tail.hpp"

#include <cmath>

namespace {

namespace iq = gr4pm::iq;
using gr4pm::cmac;

constexpr int kNt = 256;             // threads of a workgroup, and the most frames of a tile
constexpr int kGroup = 8;            // channels of a workgroup
constexpr size_t kStageItems = 8192; // complex64 items of the stage: 64 KiB
constexpr size_t kMaxK = 64, kMaxD = 1024, kMaxL = 8192;

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
    unsigned T;           // frames of a tile
    unsigned Lc;          // taps of a chunk
    unsigned RS;          // items of a stage row (odd)
    unsigned rcpD;        // ceil(2^32 / D) for D >= 2: j div D = umulhi(j, rcpD) for j < 2^13
    float scale;          // of an integer format's unpack
};

// NC: channels of this workgroup's group; F: the input's format (iq::kC64: complex64)
template <int NC, int F>
__device__ __forceinline__ void ddc_tile(const DdcArgs& a, float2* s)
{
    const unsigned tid = threadIdx.x;
    const unsigned D = a.D, L = a.L, T = a.T, RS = a.RS;
    const size_t f0 = static_cast<size_t>(blockIdx.x) * T;
    const unsigned k0 = blockIdx.y * kGroup;
    const float2* __restrict__ g = a.g + static_cast<size_t>(k0) * L;

    float2 acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = float2{0.0f, 0.0f};

    for (unsigned t0 = 0; t0 < L; t0 += a.Lc) {
        const unsigned lc = L - t0 < a.Lc ? L - t0 : a.Lc;
        // stage item j: virtual sample vb + j; frame f0 + n takes tap t from item n D + (t0 + lc - 1 - t)
        const size_t vb = static_cast<size_t>(L - 1) + f0 * D + (D - 1) - (t0 + lc - 1);
        const unsigned S = (T - 1) * D + lc;
        if (t0) __syncthreads(); // the previous chunk has been read
        for (unsigned j = tid; j < S; j += kNt) {
            const unsigned col = D == 1 ? j : __umulhi(j, a.rcpD);
            const unsigned row = j - col * D;
            const size_t v = vb + j;
            s[row * RS + col] = v < a.total ? iq::vsample<F>(a.hist, a.H, a.in, a.scale, v) : float2{0.0f, 0.0f};
        }
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
            const uint32_t phi = a.w[k0 + c] * i;
            double sn, cs;
            sincospi(-static_cast<double>(phi) * (1.0 / 2147483648.0), &sn, &cs); // the argument is exact
            const float2 r = {static_cast<float>(cs), static_cast<float>(sn)};
            float2 y = {0.0f, 0.0f};
            cmac(y, r, acc[c]);
            a.out[static_cast<size_t>(k0 + c) * a.out_stride + f] = y;
        }
    }
}

template <int F>
__global__ __launch_bounds__(kNt) void k_ddc(DdcArgs a)
{
    extern __shared__ float2 s_ddc[];
    const unsigned left = a.K - blockIdx.y * kGroup;
    switch (left < kGroup ? left : kGroup) {
    case 1: ddc_tile<1, F>(a, s_ddc); break;
    case 2: ddc_tile<2, F>(a, s_ddc); break;
    case 3: ddc_tile<3, F>(a, s_ddc); break;
    case 4: ddc_tile<4, F>(a, s_ddc); break;
    case 5: ddc_tile<5, F>(a, s_ddc); break;
    case 6: ddc_tile<6, F>(a, s_ddc); break;
    case 7: ddc_tile<7, F>(a, s_ddc); break;
    default: ddc_tile<8, F>(a, s_ddc); break;
    }
}

constexpr size_t kMaxI = 64;
constexpr unsigned kWave = 64;       // lanes of a wave, and the most items per branch of a rational tile

struct RddcArgs {
    const float2* hist;   // the P - 1 samples in front of in[0]
    const void* in;       // complex64, or items of the kernel's integer format
    float2* out;
    const float2* g;      // rotated taps, K I P items: group by group, a group's as [I][P][its channels]
    const uint32_t* w;    // [K] frequency words
    size_t H;             // P - 1
    size_t total;         // H + n_in
    size_t out_stride;
    size_t n_items;
    uint64_t pos;         // absolute index of in[0]
    uint64_t m0;          // the call's first item: its upsampled index, counted from in[0]'s
    unsigned K, D, I, L;
    unsigned P;           // ceil(L / I)
    unsigned T;           // items per branch of a tile
    unsigned RS;          // items of a stage row (odd)
    unsigned rcpD;        // as in DdcArgs
    unsigned Dinv;        // D^-1 mod I
    float scale;
};

typedef const float __attribute__((address_space(4))) * ConstTaps; // a float2 table, component by component

template <int NC, int F>
__device__ __forceinline__ void rddc_tile(const RddcArgs& a, float2* s)
{
    const unsigned tid = threadIdx.x, lane = tid & (kWave - 1);
    const unsigned wave = __builtin_amdgcn_readfirstlane(tid / kWave), waves = blockDim.x / kWave;
    const unsigned D = a.D, I = a.I, L = a.L, P = a.P, T = a.T, RS = a.RS;
    const unsigned IT = I * T;
    const size_t n0 = static_cast<size_t>(blockIdx.x) * IT; // the tile's first item
    const unsigned k0 = blockIdx.y * kGroup;
    const uint64_t m0 = a.m0 + static_cast<uint64_t>(n0) * D;
    const uint64_t c0 = m0 / I;                              // its sample, counted from in[0]
    const unsigned b0 = static_cast<unsigned>(m0 - c0 * I); // its branch
    // stage item j: virtual sample c0 + j, that is sample c0 - (P - 1) + j of the call; the tile's last item takes
    // its tap 0 from item (b0 + (I T - 1) D) div I + P - 1 < S
    const unsigned S = ((IT - 1) * D + I - 1) / I + P;
    for (unsigned j = tid; j < S; j += blockDim.x) {
        const unsigned col = D == 1 ? j : __umulhi(j, a.rcpD);
        const unsigned row = j - col * D;
        const size_t v = static_cast<size_t>(c0) + j;
        s[row * RS + col] = v < a.total ? iq::vsample<F>(a.hist, a.H, a.in, a.scale, v) : float2{0.0f, 0.0f};
    }
    __syncthreads();
    float2* so = s + RS * D; // [NC][I T]: the tile's results
    for (unsigned p = wave; p < I; p += waves) {
        // the branch's first item of the tile is item q: (b0 + q D) mod I = p; its lanes' items are q + I lane, their
        // samples D apart
        const unsigned q = (p + I - b0) % I * a.Dinv % I;
        const unsigned e = (b0 + q * D) / I;           // its sample, counted from c0
        const unsigned Pp = p < L ? (L - p + I - 1) / I : 0; // taps of h[p::I]
        const size_t n = n0 + q + static_cast<size_t>(I) * lane;
        if (lane < T && n < a.n_items) {
            // the table is written at create only: read through the constant address space, a wave-uniform address
            // there is a scalar load whatever else the kernel stores
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
                const uint32_t phi = a.w[k0 + c] * i;
                double sn, cs;
                sincospi(-static_cast<double>(phi) * (1.0 / 2147483648.0), &sn, &cs); // the argument is exact
                const float2 r = {static_cast<float>(cs), static_cast<float>(sn)};
                float2 y = {0.0f, 0.0f};
                cmac(y, r, acc[c]);
                so[c * IT + q + I * lane] = y;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NC; ++c)
        for (unsigned ti = tid; ti < IT && n0 + ti < a.n_items; ti += blockDim.x)
            a.out[static_cast<size_t>(k0 + c) * a.out_stride + n0 + ti] = so[c * IT + ti];
}

template <int F>
__global__ __launch_bounds__(kNt) void k_ddc_rational(RddcArgs a)
{
    extern __shared__ float2 s_rddc[];
    const unsigned left = a.K - blockIdx.y * kGroup;
    switch (left < kGroup ? left : kGroup) {
    case 1: rddc_tile<1, F>(a, s_rddc); break;
    case 2: rddc_tile<2, F>(a, s_rddc); break;
    case 3: rddc_tile<3, F>(a, s_rddc); break;
    case 4: rddc_tile<4, F>(a, s_rddc); break;
    case 5: rddc_tile<5, F>(a, s_rddc); break;
    case 6: rddc_tile<6, F>(a, s_rddc); break;
    case 7: rddc_tile<7, F>(a, s_rddc); break;
    default: rddc_tile<8, F>(a, s_rddc); break;
    }
}

gr4pm_status design_taps(size_t D, size_t P, double passband, double stopband, std::vector<double>& h)
{
    using gr4pm::set_error;
    if (D < 1 || D > kMaxD) {
        set_error("ddc: the decimation must be in [1, %zu], not %zu", kMaxD, D);
        return GR4PM_ERR_INVALID;
    }
    if (P < 1 || P * D > kMaxL) {
        set_error("ddc: %zu taps per phase at a decimation of %zu: the prototype has 1 .. %zu taps", P, D, kMaxL);
        return GR4PM_ERR_INVALID;
    }
    if (!gr4pm::band_edges_valid(passband, stopband, D, true)) {
        set_error("ddc: need 0 <= passband < stopband (units of the output rate) and a cutoff of at most fs / 2");
        return GR4PM_ERR_INVALID;
    }
    gr4pm::kaiser_lowpass(P * D, D, passband, stopband, h);
    return GR4PM_OK;
}

gr4pm_status design_rational_taps(size_t I, size_t D, size_t P, double passband, double stopband, std::vector<double>& h)
{
    using gr4pm::set_error;
    if (I < 1 || I > kMaxI) {
        set_error("ddc: the interpolation must be in [1, %zu], not %zu", kMaxI, I);
        return GR4PM_ERR_INVALID;
    }
    if (D < 1 || D > kMaxD) {
        set_error("ddc: the decimation must be in [1, %zu], not %zu", kMaxD, D);
        return GR4PM_ERR_INVALID;
    }
    if (P < 1 || P * D > kMaxL) {
        set_error("ddc: %zu taps per phase at a decimation of %zu: the prototype has 1 .. %zu taps", P, D, kMaxL);
        return GR4PM_ERR_INVALID;
    }
    // the cutoff, (passband + stopband) / 2 of the output rate fs I / D, within half of the output rate and half of fs
    const double most = D < I ? static_cast<double>(D) / static_cast<double>(I) : 1.0;
    if (!(passband >= 0.0 && passband < stopband && passband + stopband <= most)) {
        set_error("ddc: need 0 <= passband < stopband (units of the output rate fs %zu / %zu) and a cutoff of at most half of "
                  "the lower of the input and the output rate: passband + stopband <= %g", I, D, most);
        return GR4PM_ERR_INVALID;
    }
    gr4pm::kaiser_lowpass(P * D, D, passband, stopband, h, static_cast<double>(I));
    return GR4PM_OK;
}

} // namespace

struct gr4pm_ddc {
    size_t K = 0, D = 0, L = 0, max_frames = 0;
    unsigned T = 0, Lc = 0, RS = 0, rcpD = 0;
    size_t smem = 0;
    uint64_t start_index = 0;
    uint64_t pos = 0;       // absolute index of the first sample that is not yet part of a produced frame
    gr4pm::StreamTail tail; // L - 1 samples of history, then the incomplete frame
    hipStream_t stream = nullptr;
    std::vector<uint32_t> words;
    gr4pm::DevBuf<float2> d_g;
    gr4pm::DevBuf<uint32_t> d_w;
    // a rational handle (I > 1; L is the prototype's length, the tail keeps P - 1 samples and never a partial frame)
    size_t I = 1, P = 0;
    unsigned Dinv = 0, waves = 0;
    uint64_t taken = 0;  // samples consumed since start_index
    uint64_t next_j = 0; // the next item: its sample, counted from start_index (>= taken) ...
    unsigned next_p = 0; // ... and its branch

    void rational_start()
    {
        taken = 0;
        next_j = (D - 1) / I;
        next_p = static_cast<unsigned>((D - 1) % I);
    }
    // the next item's upsampled index counted from that of the next sample: below D + I
    uint64_t rational_m0() const { return (next_j - taken) * I + next_p; }
    // items a call of n_in samples completes: those whose sample is among them, m0 + t D < n_in I
    size_t rational_items(size_t n_in) const
    {
        const uint64_t m0 = rational_m0(), end = static_cast<uint64_t>(n_in) * I;
        return end > m0 ? static_cast<size_t>((end - m0 - 1) / D + 1) : 0;
    }
};

using namespace gr4pm;

static gr4pm_status process_rational(gr4pm_ddc* h, const void* in, int format, float scale, size_t n_in, gr4pm_c64* out,
                                     size_t out_stride, size_t out_cap_frames, size_t* n_frames)
{
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
    const size_t F = h->rational_items(n_in);
    if (F > out_cap_frames) {
        set_error("ddc: %zu items, room for %zu", F, out_cap_frames);
        return GR4PM_ERR_OVERFLOW;
    }
    if (F && (!out || (h->K > 1 && out_stride < F))) {
        set_error("ddc: no output array, or a row stride of %zu items for %zu items", out_stride, F);
        return GR4PM_ERR_INVALID;
    }
    RddcArgs a;
    a.hist = t.hist;
    a.in = in;
    a.out = reinterpret_cast<float2*>(out);
    a.g = h->d_g.p;
    a.w = h->d_w.p;
    a.H = t.H;
    a.total = t.H + n_in;
    a.out_stride = out_stride;
    a.n_items = F;
    a.pos = h->start_index + h->taken;
    a.m0 = h->rational_m0();
    a.K = static_cast<unsigned>(h->K);
    a.D = static_cast<unsigned>(D);
    a.I = static_cast<unsigned>(I);
    a.L = static_cast<unsigned>(h->L);
    a.P = static_cast<unsigned>(h->P);
    a.T = h->T;
    a.RS = h->RS;
    a.rcpD = h->rcpD;
    a.Dinv = h->Dinv;
    a.scale = scale;
    const size_t tile = I * h->T;
    const dim3 grid(static_cast<unsigned>((F + tile - 1) / tile), static_cast<unsigned>((h->K + kGroup - 1) / kGroup));
    iq::with_format(format, [&](auto f) {
        constexpr int Fm = decltype(f)::value;
        if (F) hipLaunchKernelGGL(k_ddc_rational<Fm>, grid, dim3(h->waves * kWave), h->smem, h->stream, a);
        h->tail.launch_history<Fm>(t, in, 0, n_in, scale, h->stream);
    });
    GR4PM_HIP_TRY(hipGetLastError());
    h->tail.commit(t);
    // F items on: the upsampled index by F D, in (sample, branch) form so that nothing but the sample index grows
    const uint64_t step = h->next_p + static_cast<uint64_t>(F) * D;
    h->next_j += step / I;
    h->next_p = static_cast<unsigned>(step % I);
    h->taken += n_in;
    *n_frames = F;
    return GR4PM_OK;
}

// process() and process_iq(): format iq::kC64 for complex64 samples
static gr4pm_status process_any(gr4pm_ddc* h, const void* in, int format, float scale, size_t n_in, gr4pm_c64* out,
                                size_t out_stride, size_t out_cap_frames, size_t* n_frames)
{
    if (!h || !n_frames) return GR4PM_ERR_INVALID;
    *n_frames = 0;
    if (h->I > 1) return process_rational(h, in, format, scale, n_in, out, out_stride, out_cap_frames, n_frames);
    if (n_in > h->max_frames * h->D) {
        set_error("ddc: %zu items, the handle was made for %zu frames of %zu", n_in, h->max_frames, h->D);
        return GR4PM_ERR_OVERFLOW;
    }
    if (n_in == 0) return GR4PM_OK;
    if (!in) {
        set_error("ddc: no input array");
        return GR4PM_ERR_INVALID;
    }
    const size_t D = h->D, L = h->L;
    const StreamTail::Plan t = h->tail.plan(n_in);
    const size_t F = t.n_frames;
    if (F > out_cap_frames) {
        set_error("ddc: %zu frames, room for %zu", F, out_cap_frames);
        return GR4PM_ERR_OVERFLOW;
    }
    if (F && (!out || (h->K > 1 && out_stride < F))) {
        set_error("ddc: no output array, or a row stride of %zu items for %zu frames", out_stride, F);
        return GR4PM_ERR_INVALID;
    }
    DdcArgs a;
    a.hist = t.hist;
    a.in = in;
    a.out = reinterpret_cast<float2*>(out);
    a.g = h->d_g.p;
    a.w = h->d_w.p;
    a.H = t.H;
    a.total = t.H + n_in;
    a.out_stride = out_stride;
    a.n_frames = F;
    a.pos = h->pos;
    a.K = static_cast<unsigned>(h->K);
    a.D = static_cast<unsigned>(D);
    a.L = static_cast<unsigned>(L);
    a.T = h->T;
    a.Lc = h->Lc;
    a.RS = h->RS;
    a.rcpD = h->rcpD;
    a.scale = scale;
    const dim3 grid(static_cast<unsigned>((F + h->T - 1) / h->T), static_cast<unsigned>((h->K + kGroup - 1) / kGroup));
    iq::with_format(format, [&](auto f) {
        constexpr int Fm = decltype(f)::value;
        if (F) hipLaunchKernelGGL(k_ddc<Fm>, grid, dim3(kNt), h->smem, h->stream, a);
        h->tail.launch_history<Fm>(t, in, 0, n_in, scale, h->stream);
    });
    GR4PM_HIP_TRY(hipGetLastError());
    h->tail.commit(t);
    h->pos += static_cast<uint64_t>(F) * D;
    *n_frames = F;
    return GR4PM_OK;
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
    const size_t K = p->n_channels, D = p->decimation;
    std::vector<uint32_t> words;
    GR4PM_TRY(frequency_words("ddc", p->frequencies, K, kMaxK, words));
    if (D < 1 || D > kMaxD) {
        set_error("ddc: the decimation must be in [1, %zu], not %zu", kMaxD, D);
        return GR4PM_ERR_INVALID;
    }
    if (p->max_frames == 0 || p->max_frames > (size_t(1) << 31)) {
        set_error("ddc: max_frames must be in [1, 2^31]");
        return GR4PM_ERR_INVALID;
    }
    if (p->taps && (p->n_taps < 1 || p->n_taps > kMaxL)) {
        set_error("ddc: the prototype has 1 .. %zu taps, not %zu", kMaxL, p->n_taps);
        return GR4PM_ERR_INVALID;
    }
    std::vector<float> taps;
    GR4PM_TRY(taps_or_design(p->taps, p->n_taps, [&](std::vector<double>& hd) { return design_taps(D, 12, 0.25, 0.75, hd); }, taps));
    const size_t L = taps.size();
    GR4PM_TRY(require_device());
    std::unique_ptr<gr4pm_ddc> h(new (std::nothrow) gr4pm_ddc);
    if (!h) return GR4PM_ERR_NOMEM;
    h->K = K;
    h->D = D;
    h->L = L;
    h->max_frames = p->max_frames;
    h->start_index = h->pos = p->start_index;
    h->stream = static_cast<hipStream_t>(p->stream);
    // the tile: rows of `cols` items (made odd), D rows within the stage; a tile of T frames and a chunk of Lc taps
    // use T + (Lc - 1) div D columns.  All of L in one chunk where 256 frames leave room for it, else half the columns
    // go to frames and the rest to taps.
    size_t cols = kStageItems / D;
    if (cols % 2 == 0) --cols; // >= 7
    const size_t extra_all = (L - 1) / D;
    size_t T = kNt, extra = extra_all;
    if (T + extra_all > cols) {
        T = cols / 2 < static_cast<size_t>(kNt) ? cols / 2 : static_cast<size_t>(kNt);
        extra = cols - T < extra_all ? cols - T : extra_all;
    }
    h->T = static_cast<unsigned>(T);
    h->Lc = static_cast<unsigned>((extra + 1) * D < L ? (extra + 1) * D : L);
    h->RS = static_cast<unsigned>((T + extra) | 1);
    h->rcpD = reciprocal_word(D);
    h->smem = static_cast<size_t>(h->RS) * D * sizeof(float2);

    h->words = std::move(words);
    std::vector<float2> g(K * L);
    for (size_t k = 0; k < K; ++k) {
        const uint32_t w = h->words[k];
        // a group's taps interleaved by channel: tap t of all its channels side by side
        const size_t k0 = k / kGroup * kGroup, nc = K - k0 < static_cast<size_t>(kGroup) ? K - k0 : static_cast<size_t>(kGroup);
        for (size_t t = 0; t < L; ++t) {
            g[k0 * L + t * nc + (k - k0)] = rotated_tap(static_cast<double>(taps[t]), w * static_cast<uint32_t>(t));
        }
    }
    GR4PM_TRY(h->d_g.alloc(K * L));
    GR4PM_TRY(h->d_w.alloc(K));
    GR4PM_TRY(h->tail.alloc(L - 1, D, 1, h->stream));
    GR4PM_TRY(h->d_g.upload(g.data(), g.size(), h->stream));
    GR4PM_TRY(h->d_w.upload(h->words.data(), K, h->stream));
    if (h->smem > 48 * 1024)
        GR4PM_TRY(raise_dynamic_lds({reinterpret_cast<const void*>(&k_ddc<iq::kC64>), reinterpret_cast<const void*>(&k_ddc<GR4PM_IQ_SC16>),
                                     reinterpret_cast<const void*>(&k_ddc<GR4PM_IQ_SC8>), reinterpret_cast<const void*>(&k_ddc<GR4PM_IQ_CU8>)},
                                    kStageItems * sizeof(float2), "ddc"));
    return finish_create(h, out, "ddc");
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
    const size_t K = p->n_channels, D = p->decimation, I = p->interpolation;
    if (I < 1 || I > kMaxI) {
        set_error("ddc: the interpolation must be in [1, %zu], not %zu", kMaxI, I);
        return GR4PM_ERR_INVALID;
    }
    if (I == 1) { // the integer Ddc, with its own kernel
        const gr4pm_ddc_params q = {K, D, p->frequencies, p->taps, p->n_taps, p->max_frames, p->start_index, p->stream};
        return gr4pm_ddc_create(&q, out);
    }
    std::vector<uint32_t> words;
    GR4PM_TRY(frequency_words("ddc", p->frequencies, K, kMaxK, words));
    if (D < 1 || D > kMaxD) {
        set_error("ddc: the decimation must be in [1, %zu], not %zu", kMaxD, D);
        return GR4PM_ERR_INVALID;
    }
    size_t gcd = I;
    for (size_t b = D % I; b;) {
        const size_t r = gcd % b;
        gcd = b, b = r;
    }
    if (gcd != 1) {
        set_error("ddc: the ratio %zu / %zu is not in lowest terms: use %zu / %zu", I, D, I / gcd, D / gcd);
        return GR4PM_ERR_INVALID;
    }
    if (p->max_frames == 0 || p->max_frames > (size_t(1) << 31)) {
        set_error("ddc: max_frames must be in [1, 2^31]");
        return GR4PM_ERR_INVALID;
    }
    if (p->taps && (p->n_taps < 1 || p->n_taps > kMaxL)) {
        set_error("ddc: the prototype has 1 .. %zu taps, not %zu", kMaxL, p->n_taps);
        return GR4PM_ERR_INVALID;
    }
    std::vector<float> taps;
    GR4PM_TRY(taps_or_design(p->taps, p->n_taps, [&](std::vector<double>& hd) { return design_rational_taps(I, D, 12, 0.25, 0.75, hd); },
                             taps));
    const size_t L = taps.size(), P = (L + I - 1) / I;
    GR4PM_TRY(require_device());
    std::unique_ptr<gr4pm_ddc> h(new (std::nothrow) gr4pm_ddc);
    if (!h) return GR4PM_ERR_NOMEM;
    h->K = K;
    h->D = D;
    h->L = L;
    h->I = I;
    h->P = P;
    h->max_frames = p->max_frames;
    h->start_index = h->pos = p->start_index;
    h->stream = static_cast<hipStream_t>(p->stream);
    h->rational_start();
    for (size_t v = 1; v < I; ++v)
        if (v * D % I == 1) h->Dinv = static_cast<unsigned>(v);
    // waves of a workgroup: a wave takes a branch at a time, so the count w of 2 .. 4 with the fewest wave slots
    // ceil(I / w) w, the larger one of equals
    size_t waves = 2;
    for (size_t w = 3; w <= kNt / kWave; ++w)
        if ((I + w - 1) / w * w <= (I + waves - 1) / waves * waves) waves = w;
    h->waves = static_cast<unsigned>(waves);
    // the tile: the most items per branch T <= 64 whose stage (D rows of an odd number of items for the
    // ((I T - 1) D + I - 1) div I + P samples that I T consecutive items reach) and results (I T per channel of a
    // group) fit the 64 KiB
    const size_t G = K < static_cast<size_t>(kGroup) ? K : static_cast<size_t>(kGroup);
    size_t T = kWave, RS = 0;
    for (;; --T) {
        if (T == 0) {
            set_error("ddc: no tile of %zu / %zu with %zu taps fits the stage", I, D, L);
            return GR4PM_ERR_INVALID;
        }
        const size_t S = ((I * T - 1) * D + I - 1) / I + P;
        RS = ((S + D - 1) / D) | 1;
        if (RS * D + I * T * G <= kStageItems) break;
    }
    h->T = static_cast<unsigned>(T);
    h->RS = static_cast<unsigned>(RS);
    h->rcpD = reciprocal_word(D);
    h->smem = (RS * D + I * T * G) * sizeof(float2);

    h->words = std::move(words);
    std::vector<float2> g(K * I * P, float2{0.0f, 0.0f});
    for (size_t k = 0; k < K; ++k) {
        const uint32_t w = h->words[k];
        // a group's taps as [branch][s][channel]: tap s of a branch for all its channels side by side
        const size_t k0 = k / kGroup * kGroup, nc = K - k0 < static_cast<size_t>(kGroup) ? K - k0 : static_cast<size_t>(kGroup);
        for (size_t t = 0; t < L; ++t) {
            const size_t br = t % I, s = t / I;
            g[k0 * I * P + (br * P + s) * nc + (k - k0)] = rotated_tap(static_cast<double>(taps[t]), w * static_cast<uint32_t>(s));
        }
    }
    GR4PM_TRY(h->d_g.alloc(g.size()));
    GR4PM_TRY(h->d_w.alloc(K));
    GR4PM_TRY(h->tail.alloc(P - 1, 1, 1, h->stream));
    GR4PM_TRY(h->d_g.upload(g.data(), g.size(), h->stream));
    GR4PM_TRY(h->d_w.upload(h->words.data(), K, h->stream));
    if (h->smem > 48 * 1024)
        GR4PM_TRY(raise_dynamic_lds({reinterpret_cast<const void*>(&k_ddc_rational<iq::kC64>), reinterpret_cast<const void*>(&k_ddc_rational<GR4PM_IQ_SC16>),
                                     reinterpret_cast<const void*>(&k_ddc_rational<GR4PM_IQ_SC8>), reinterpret_cast<const void*>(&k_ddc_rational<GR4PM_IQ_CU8>)},
                                    kStageItems * sizeof(float2), "ddc"));
    return finish_create(h, out, "ddc");
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
    h->pos = h->start_index;
    if (h->I > 1) h->rational_start();
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_ddc_output_items(const gr4pm_ddc* h, size_t n_in, size_t* n_frames)
try {
    if (!h || !n_frames) return GR4PM_ERR_INVALID;
    *n_frames = h->I > 1 ? h->rational_items(n_in) : h->tail.frames(n_in);
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

} // extern "C"
