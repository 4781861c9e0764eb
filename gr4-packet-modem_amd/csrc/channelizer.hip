// channelizer.hip -- critically sampled polyphase analysis bank: one wideband c64 stream to M baseband channels at
// 1/M of the rate, channel-major (out[k][n], the layout gr4pm_multichannel_receiver_submit takes).  The project's own
// block (the reference is a one-channel modem).  Definition (include/gr4pm_hip.h):
//     y_k[n] = sum_t h[t] x[n M + M - 1 - t] exp(-2 pi j k (n M + M - 1 - t) / M),   x[i] = 0 for i < 0
// With t = p M + M - 1 - m the phase depends on m alone, so
//     u_n[m] = sum_p h[p M + M - 1 - m] x[(n - p) M + m]      (branch sums, p = 0 .. P-1 in that order)
//     y_k[n] = sum_m u_n[m] exp(-2 pi j k m / M)              (one forward M-point DFT per frame)
//
// k_channelize: a workgroup owns T = 4096 / M consecutive frames.
//   fast form (M = 16, 64, 256; LDS within 64 KiB): the (T + P - 1) M samples it needs go to LDS once (rows of M + 1 items:
//     the odd row stride keeps the transposed read at the end free of bank conflicts); every thread holds one branch
//     m and 16 frames, so a tap is loaded once per 16 products; the branch sums replace the staged rows in place.
//   generic form (any M up to 1024, any P up to 32, or GR4PM_CHANNELIZER=generic at create): the branch sums read the
//     samples from global memory and only the T frames live in LDS.
//   Both: decimation-in-frequency radix-2 levels in place in LDS (the fast form does two levels per pass on four
//   points in registers -- the same butterflies with the same operands, so the two forms agree bit for bit), twiddles
//   from a table made in double at create; then channel k's T items leave as one contiguous run, lanes on consecutive
//   items of the row, read from LDS at the bit-reversed column.
// Every product and sum rounds on its own (EXACT_FLAGS) in an order that depends on (frame, branch) only: a result
// does not depend on how the stream is cut into calls.
// The stream's tail -- the last (P - 1) M samples plus the incomplete frame -- is stream_tail.hpp's: its kernel moves it
// to the handle's other history buffer.
// Integer input (gr4pm_channelizer_process_iq): both kernels are templated on the input format and convert where a
// sample enters them -- the load into the stage, vsample(), the history's tail -- with iq_format.hpp's unpack_item(),
// the very expression gr4pm_iq_unpack evaluates.  The stage, the history and everything behind them stay complex64, so
// the result is that of process() on the unpacked samples bit for bit, and calls of any format mix on one handle.
#include "kaiser_design.hpp"
#include "stream_tail.hpp"

#include <cmath>
#include <cstdlib>

namespace {

namespace iq = gr4pm::iq;

constexpr int kNt = 256;              // threads of a workgroup
constexpr int kPoints = 4096;         // frame samples a workgroup transforms: T = kPoints / M frames
constexpr int kPer = kPoints / kNt;   // branch sums per thread
constexpr size_t kFastSmem = 64 * 1024;
constexpr size_t kMaxM = 1024, kMaxP = 32;

struct ChanArgs {
    const float2* hist;     // the H samples in front of in[0]: (P - 1) M of history, then the carried partial frame
    const void* in;         // complex64, or items of the kernel's integer format
    float2* out;
    const float* taps_r;    // [P][M]: taps_r[p M + m] = h[p M + M - 1 - m]
    const float2* twiddle;  // [M / 2]: exp(-2 pi j i / M)
    const unsigned* select; // rows to write, or null: all M in order
    size_t H;
    size_t out_stride;
    size_t n_frames;
    unsigned n_rows;
    unsigned P;
    unsigned lm;            // log2 M
    float scale;            // of an integer format's unpack
};

__device__ __forceinline__ void tap(float2& acc, float h, float2 x)
{
    acc.x = acc.x + h * x.x;
    acc.y = acc.y + h * x.y;
}

// a, b -> a + b, (a - b) w
__device__ __forceinline__ void bfly(float2& a, float2& b, float2 w)
{
    const float2 s = {a.x + b.x, a.y + b.y};
    const float2 d = {a.x - b.x, a.y - b.y};
    a = s;
    b = float2{d.x * w.x - d.y * w.y, d.x * w.y + d.y * w.x};
}

// LM: log2 M of the fast form (even), 0: the generic form (a.lm); F: the input's format (iq::kC64: complex64)
template <int LM, int F>
__global__ __launch_bounds__(kNt) void k_channelize(ChanArgs a)
{
    extern __shared__ float2 s_ch[];
    const unsigned lm = LM ? LM : a.lm;
    const unsigned M = 1u << lm, T = kPoints >> lm, RS = M + 1, P = a.P;
    const unsigned t = threadIdx.x;
    const size_t f0 = static_cast<size_t>(blockIdx.x) * T;
    const unsigned Tw = a.n_frames - f0 < T ? static_cast<unsigned>(a.n_frames - f0) : T;
    float2* s_tw = s_ch;                       // M / 2 twiddles
    float2* s = s_ch + M / 2;                  // rows of RS items
    for (unsigned i = t; i < M / 2; i += kNt) s_tw[i] = a.twiddle[i];

    float2 acc[kPer];
#pragma unroll
    for (int o = 0; o < kPer; ++o) acc[o] = float2{0.0f, 0.0f};
    if constexpr (LM != 0) {
        // row r of the stage: frame f0 + r of the stream that starts (P - 1) frames before this call's first frame
        const unsigned rows = Tw + P - 1;
        for (unsigned i = t; i < (T + P - 1) * M; i += kNt) {
            const unsigned r = i >> lm, m = i & (M - 1);
            s[r * RS + m] = r < rows ? iq::vsample<F>(a.hist, a.H, a.in, a.scale, (f0 + r) * M + m) : float2{0.0f, 0.0f};
        }
        __syncthreads();
        const unsigned m = t & (M - 1), n0 = t >> lm; // kNt is a multiple of M: one branch per thread
        for (unsigned p = 0; p < P; ++p) {
            const float h = a.taps_r[p * M + m];
            const float2* col = s + (n0 + P - 1 - p) * RS + m;
#pragma unroll
            for (int o = 0; o < kPer; ++o) tap(acc[o], h, col[o * (kNt >> LM) * RS]);
        }
        __syncthreads(); // the stage has been read: the branch sums take its place
#pragma unroll
        for (int o = 0; o < kPer; ++o) s[(n0 + o * (kNt >> LM)) * RS + m] = acc[o];
    } else {
#pragma unroll
        for (int o = 0; o < kPer; ++o) {
            const unsigned idx = o * kNt + t, n = idx >> lm, m = idx & (M - 1);
            if (n < Tw)
                for (unsigned p = 0; p < P; ++p)
                    tap(acc[o], a.taps_r[p * M + m], iq::vsample<F>(a.hist, a.H, a.in, a.scale, (f0 + n + P - 1 - p) * M + m));
            s[n * RS + m] = acc[o];
        }
    }
    __syncthreads();

    if constexpr (LM != 0) {
#pragma unroll
        for (int lvl = 0; lvl < LM; lvl += 2) {
            const unsigned lh = LM - 1 - lvl, h = 1u << lh, hh = h >> 1;
#pragma unroll
            for (int e = 0; e < kPoints / 4 / kNt; ++e) {
                const unsigned q = e * kNt + t, n = q >> (LM - 2), r = q & (M / 4 - 1);
                const unsigned g = r >> (lh - 1), j = r & (hh - 1);
                float2* v = s + n * RS + (g << (lh + 1)) + j;
                float2 a0 = v[0], a1 = v[hh], a2 = v[h], a3 = v[h + hh];
                const float2 w2 = s_tw[j << (lvl + 1)];
                bfly(a0, a2, s_tw[j << lvl]);
                bfly(a1, a3, s_tw[(j + hh) << lvl]);
                bfly(a0, a1, w2);
                bfly(a2, a3, w2);
                v[0] = a0, v[hh] = a1, v[h] = a2, v[h + hh] = a3;
            }
            __syncthreads();
        }
    } else {
        for (unsigned lvl = 0; lvl < lm; ++lvl) {
            const unsigned lh = lm - 1 - lvl, h = 1u << lh;
#pragma unroll
            for (int e = 0; e < kPoints / 2 / kNt; ++e) {
                const unsigned q = e * kNt + t, n = q >> (lm - 1), r = q & (M / 2 - 1);
                const unsigned g = r >> lh, j = r & (h - 1);
                float2* v = s + n * RS + (g << (lh + 1)) + j;
                float2 a0 = v[0], a1 = v[h];
                bfly(a0, a1, s_tw[j << lvl]);
                v[0] = a0, v[h] = a1;
            }
            __syncthreads();
        }
    }

    // X[k] of frame n sits at column bitrev(k); consecutive lanes take consecutive items of one output row
    const unsigned lt = 12 - lm; // log2 T
    for (unsigned idx = t; idx < a.n_rows * T; idx += kNt) {
        const unsigned n = idx & (T - 1), ks = idx >> lt;
        if (n >= Tw) continue;
        const unsigned k = a.select ? a.select[ks] : ks;
        const unsigned rev = __brev(k) >> (32 - lm);
        a.out[static_cast<size_t>(ks) * a.out_stride + f0 + n] = s[n * RS + rev];
    }
}

bool power_of_two_in_range(size_t M) { return M >= 2 && M <= kMaxM && (M & (M - 1)) == 0; }

size_t smem_fast(size_t M, size_t P) { return (M / 2 + (kPoints / M + P - 1) * (M + 1)) * sizeof(float2); }
size_t smem_generic(size_t M) { return (M / 2 + (kPoints / M) * (M + 1)) * sizeof(float2); }

gr4pm_status check_shape(size_t M, size_t P)
{
    using gr4pm::set_error;
    if (!power_of_two_in_range(M)) {
        set_error("channelizer: M must be a power of two in [2, %zu], not %zu", kMaxM, M);
        return GR4PM_ERR_INVALID;
    }
    if (P < 1 || P > kMaxP) {
        set_error("channelizer: taps per branch must be in [1, %zu], not %zu", kMaxP, P);
        return GR4PM_ERR_INVALID;
    }
    return GR4PM_OK;
}

// the checks of the channelizer's design; the design itself is kaiser_design.hpp's (shared with ddc.hip)
gr4pm_status design_taps(size_t M, size_t P, double passband, double stopband, std::vector<double>& h)
{
    GR4PM_TRY(check_shape(M, P));
    if (!gr4pm::band_edges_valid(passband, stopband, M, false)) {
        gr4pm::set_error("channelizer: need 0 <= passband < stopband (units of the channel spacing) and a cutoff below fs / 2");
        return GR4PM_ERR_INVALID;
    }
    gr4pm::kaiser_lowpass(P * M, M, passband, stopband, h);
    return GR4PM_OK;
}

template <int F>
const void* channelize_fn(bool fast, size_t M)
{
    return !fast ? reinterpret_cast<const void*>(&k_channelize<0, F>)
                 : (M == 16 ? reinterpret_cast<const void*>(&k_channelize<4, F>)
                            : (M == 64 ? reinterpret_cast<const void*>(&k_channelize<6, F>)
                                       : reinterpret_cast<const void*>(&k_channelize<8, F>)));
}

} // namespace

struct gr4pm_channelizer {
    size_t M = 0, P = 0, max_frames = 0;
    unsigned lm = 0, n_rows = 0;
    bool fast = false, selected = false;
    gr4pm::StreamTail tail; // (P - 1) M samples of history, then the incomplete frame
    hipStream_t stream = nullptr;
    gr4pm::DevBuf<float> d_taps;
    gr4pm::DevBuf<float2> d_twiddle;
    gr4pm::DevBuf<unsigned> d_select;
};

using namespace gr4pm;

// process() and process_iq(): format iq::kC64 for complex64 samples
static gr4pm_status process_any(gr4pm_channelizer* h, const void* in, int format, float scale, size_t n_in, gr4pm_c64* out,
                                size_t out_stride, size_t out_cap_frames, size_t* n_frames)
{
    if (!h || !n_frames) return GR4PM_ERR_INVALID;
    *n_frames = 0;
    if (n_in > h->max_frames * h->M) {
        set_error("channelizer: %zu items, the handle was made for %zu frames of %zu", n_in, h->max_frames, h->M);
        return GR4PM_ERR_OVERFLOW;
    }
    if (n_in == 0) return GR4PM_OK;
    if (!in) {
        set_error("channelizer: no input array");
        return GR4PM_ERR_INVALID;
    }
    const size_t M = h->M, P = h->P;
    const StreamTail::Plan t = h->tail.plan(n_in);
    const size_t F = t.n_frames;
    if (F > out_cap_frames) {
        set_error("channelizer: %zu frames, room for %zu", F, out_cap_frames);
        return GR4PM_ERR_OVERFLOW;
    }
    if (F && (!out || (h->n_rows > 1 && out_stride < F))) {
        set_error("channelizer: no output array, or a row stride of %zu items for %zu frames", out_stride, F);
        return GR4PM_ERR_INVALID;
    }
    ChanArgs a;
    a.hist = t.hist;
    a.in = in;
    a.out = reinterpret_cast<float2*>(out);
    a.taps_r = h->d_taps.p;
    a.twiddle = h->d_twiddle.p;
    a.select = h->selected ? h->d_select.p : nullptr;
    a.H = t.H;
    a.out_stride = out_stride;
    a.n_frames = F;
    a.n_rows = h->n_rows;
    a.P = static_cast<unsigned>(P);
    a.lm = h->lm;
    a.scale = scale;
    const size_t T = kPoints / M;
    const dim3 grid(static_cast<unsigned>((F + T - 1) / T));
    const size_t smem = h->fast ? smem_fast(M, P) : smem_generic(M);
    iq::with_format(format, [&](auto f) {
        constexpr int Fm = decltype(f)::value;
        if (F) {
            void* args[] = {&a};
            (void)hipLaunchKernel(channelize_fn<Fm>(h->fast, M), grid, dim3(kNt), args, smem, h->stream);
        }
        h->tail.launch_history<Fm>(t, in, 0, n_in, scale, h->stream);
    });
    GR4PM_HIP_TRY(hipGetLastError());
    h->tail.commit(t);
    *n_frames = F;
    return GR4PM_OK;
}

extern "C" {

gr4pm_status gr4pm_channelizer_taps(size_t n_channels, size_t taps_per_branch, double passband, double stopband, float* out)
try {
    if (!out) return GR4PM_ERR_INVALID;
    std::vector<double> h;
    GR4PM_TRY(design_taps(n_channels, taps_per_branch, passband, stopband, h));
    round_taps(h, out);
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_channelizer_create(const gr4pm_channelizer_params* p, gr4pm_channelizer** out)
try {
    if (!p || !out) return GR4PM_ERR_INVALID;
    *out = nullptr;
    const size_t M = p->n_channels, P = p->taps_per_branch;
    GR4PM_TRY(check_shape(M, P));
    if (p->max_frames == 0 || p->max_frames > (size_t(1) << 31)) {
        set_error("channelizer: max_frames must be in [1, 2^31]");
        return GR4PM_ERR_INVALID;
    }
    if (p->n_select > M || (p->n_select && !p->select)) {
        set_error("channelizer: %zu selected rows of %zu channels", p->n_select, M);
        return GR4PM_ERR_INVALID;
    }
    std::vector<unsigned> sel(p->n_select);
    {
        std::vector<char> seen(M, 0);
        for (size_t i = 0; i < p->n_select; ++i) {
            const uint32_t k = p->select[i];
            if (k >= M || seen[k]) {
                set_error("channelizer: select[%zu] = %u is %s", i, k, k >= M ? "not a channel" : "a duplicate");
                return GR4PM_ERR_INVALID;
            }
            seen[k] = 1;
            sel[i] = k;
        }
    }
    std::vector<float> taps;
    GR4PM_TRY(taps_or_design(p->taps, P * M, [&](std::vector<double>& hd) { return design_taps(M, P, 0.25, 0.75, hd); }, taps));
    GR4PM_TRY(require_device());
    std::unique_ptr<gr4pm_channelizer> h(new (std::nothrow) gr4pm_channelizer);
    if (!h) return GR4PM_ERR_NOMEM;
    h->M = M;
    h->P = P;
    h->max_frames = p->max_frames;
    while ((size_t(1) << h->lm) < M) ++h->lm;
    h->selected = p->n_select != 0;
    h->n_rows = static_cast<unsigned>(h->selected ? p->n_select : M);
    h->stream = static_cast<hipStream_t>(p->stream);
    const char* form = std::getenv("GR4PM_CHANNELIZER"); // "generic": the generic form also where the fast one is built
    h->fast = (M == 16 || M == 64 || M == 256) && smem_fast(M, P) <= kFastSmem && !(form && !strcmp(form, "generic"));
    if (form && *form && strcmp(form, "generic") && strcmp(form, "fast")) {
        set_error("channelizer: GR4PM_CHANNELIZER=%s (generic or fast)", form);
        return GR4PM_ERR_INVALID;
    }

    std::vector<float> taps_r(P * M);
    for (size_t q = 0; q < P; ++q)
        for (size_t m = 0; m < M; ++m) taps_r[q * M + m] = taps[q * M + M - 1 - m];
    std::vector<float2> tw(M / 2);
    for (size_t i = 0; i < M / 2; ++i) {
        const double ang = -2.0 * 3.14159265358979323846 * static_cast<double>(i) / static_cast<double>(M);
        tw[i] = float2{static_cast<float>(std::cos(ang)), static_cast<float>(std::sin(ang))};
    }
    // exact where the angle is a multiple of pi / 2 (cos(pi / 2) in double is 6e-17, not 0)
    tw[0] = float2{1.0f, 0.0f};
    if (M >= 4) tw[M / 4] = float2{0.0f, -1.0f};
    GR4PM_TRY(h->d_taps.alloc(P * M));
    GR4PM_TRY(h->d_twiddle.alloc(M / 2));
    GR4PM_TRY(h->d_select.alloc(sel.size()));
    GR4PM_TRY(h->tail.alloc((P - 1) * M, M, 1, h->stream));
    GR4PM_TRY(h->d_taps.upload(taps_r.data(), taps_r.size(), h->stream));
    GR4PM_TRY(h->d_twiddle.upload(tw.data(), tw.size(), h->stream));
    if (!sel.empty()) GR4PM_TRY(h->d_select.upload(sel.data(), sel.size(), h->stream));
    if ((h->fast ? smem_fast(M, P) : smem_generic(M)) > 48 * 1024)
        GR4PM_TRY(raise_dynamic_lds({channelize_fn<iq::kC64>(h->fast, M), channelize_fn<GR4PM_IQ_SC16>(h->fast, M),
                                     channelize_fn<GR4PM_IQ_SC8>(h->fast, M), channelize_fn<GR4PM_IQ_CU8>(h->fast, M)},
                                    kFastSmem, "channelizer"));
    return finish_create(h, out, "channelizer");
}
GR4PM_ABI_CATCH

void gr4pm_channelizer_destroy(gr4pm_channelizer* h)
try {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    delete h;
}
GR4PM_ABI_CATCH_VOID

gr4pm_status gr4pm_channelizer_reset(gr4pm_channelizer* h)
try {
    if (!h) return GR4PM_ERR_INVALID;
    return h->tail.reset(h->stream);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_channelizer_output_items(const gr4pm_channelizer* h, size_t n_in, size_t* n_frames)
try {
    if (!h || !n_frames) return GR4PM_ERR_INVALID;
    *n_frames = h->tail.frames(n_in);
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_channelizer_process(gr4pm_channelizer* h, const gr4pm_c64* in, size_t n_in, gr4pm_c64* out,
                                       size_t out_stride, size_t out_cap_frames, size_t* n_frames)
try {
    return process_any(h, in, iq::kC64, 0.0f, n_in, out, out_stride, out_cap_frames, n_frames);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_channelizer_process_iq(gr4pm_channelizer* h, const void* in, int format, float scale, size_t n_in,
                                          gr4pm_c64* out, size_t out_stride, size_t out_cap_frames, size_t* n_frames)
try {
    if (!iq::valid(format)) {
        set_error("channelizer: format %d is none of GR4PM_IQ_SC16 / SC8 / CU8", format);
        return GR4PM_ERR_INVALID;
    }
    return process_any(h, in, format, scale == 0.0f ? iq::default_scale(format) : scale, n_in, out, out_stride, out_cap_frames,
                       n_frames);
}
GR4PM_ABI_CATCH

} // extern "C"
