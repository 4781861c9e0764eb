// duc.hip -- tunable up-converter: K complex64 rows at fs / I become one wideband stream at fs, every row interpolated
// by the integer I through one real prototype and mixed to a frequency of its own; the mirror of ddc.hip.  The project's
// own block (the reference is a one-channel modem).  Definition (include/gr4pm_hip.h):
//     w_k = llrint(f_k 2^32) mod 2^32,   phi_k(i) = (w_k i) mod 2^32  (wrapping unsigned arithmetic, exact anywhere)
//     x[i] = sum_k a_k exp(+2 pi j phi_k(i) / 2^32) sum_{p : p I + r < L} h[p I + r] v_k[m - p]
//     i = start_index + m I + r,  0 <= r < I,  v_k = 0 before the start
// evaluated in the rotated-taps form
//     g_k[t] = a_k h[t] exp(+2 pi j phi_k(t) / 2^32)      (host, double, rounded to float once: Ddc's table times a_k)
//     q_k[m'] = exp(+2 pi j phi_k(start_index + m' I) / 2^32)   (device, double sincospi of phi / 2^31, rounded to float)
//     z_k[m'] = q_k[m'] v_k[m']                            (four fmaf from zero)
//     x[i] = sum_k sum_p g_k[p I + r] z_k[m - p]           (one accumulator, k ascending outside, p ascending inside)
//
// k_duc<R> (g: the rotated taps [K][P][IP], zero where p I + r >= L or r >= I; a parameter of its own so that it can
//   be __restrict__): a workgroup owns T consecutive frames m, that is the T I consecutive output samples m I + r.  A lane owns one
//   frame and R consecutive phases r (R = 1, 2, 4 or 8, the largest power of two within I), so a wave's taps
//   g_k[p I + r0 .. r0 + R) are the same address in every lane -- one aggregate load per (k, p) from a table the host
//   lays out as [k][p][phase], phases padded to a multiple of R -- and one LDS read of z_k[m - p] feeds R complex MACs
//   in registers.  T <= 256 shrinks with I so that the tile stays near 2048 samples; its 256 threads are T / 64 waves
//   of frames times 4 / (T / 64) wave-uniform phase blocks, and a wave loops over the phase blocks left.
//   The z items a tile needs go to LDS once per channel group, rotated on the way in: one sincospi per staged INPUT
//   item.  All K channels sum into one sample, so the channel groups (as many channels as fit 2048 staged items) run one
//   after the other inside the workgroup and the accumulators rest in an LDS tile [phase][frame] between them; where
//   P alone exceeds the stage a group is one channel and the p loop runs over re-staged chunks.  Either way a sample
//   sees k ascending and, within k, p ascending: groups and chunks change no bit.  The tile's row stride is odd: the
//   accumulating lanes (consecutive frames of one phase) and the storing lanes (consecutive samples, so consecutive
//   phases) both hit distinct banks, and the tile leaves as 16-byte stores contiguous across the workgroup.
// A result is a function of (absolute output index, the rows' streams) only: not of call or tile sizes.
// The rows' tails -- the last P - 1 items of each -- are stream_tail.hpp's: its kernel moves them to the handle's other
// history buffer.
#include "freq_xlate.hpp"
#include "kaiser_design.hpp"
#include "stream_tail.hpp"

#include <cmath>

namespace {

using gr4pm::cmac;

constexpr int kNt = 256;             // threads of a workgroup, and the most frames of a tile
constexpr size_t kTileItems = 2048;  // output samples of a tile, about
constexpr size_t kStageItems = 2048; // complex64 items of the stage: 16 KiB
constexpr size_t kMaxK = 64, kMaxI = 1024, kMaxL = 8192;

struct DucArgs {
    const float2* hist;  // [K][P - 1]: the items in front of in[k][0]
    const float2* in;    // row k at in + k in_stride
    float2* out;
    const uint32_t* w;   // [K] frequency words
    size_t in_stride, n_in, n_out;
    uint32_t pos;        // absolute index of this call's first output sample: the low 32 bits are all the phase needs
    unsigned K, I, L, P;
    unsigned IP;         // phases of the table and rows of the tile: I rounded up to a multiple of R
    unsigned T, TS;      // frames of a tile; items of a tile row (odd)
    unsigned WF;         // waves that share the tile's frames: 1, 2 or 4
    unsigned G;          // channels of a group
    unsigned Pc;         // taps per phase of a chunk (P unless G == 1)
    unsigned ZS;         // items of a stage row: T + Pc - 1
    unsigned rcpI;       // ceil(2^32 / I) for I >= 2: j div I = umulhi(j, rcpI) for j < 2^13
    unsigned vec;        // out is 16-byte aligned: the tile leaves two samples per store
};

template <int R>
struct TapBlock {
    float2 v[R];
};

template <int R>
__global__ __launch_bounds__(kNt) void k_duc(DucArgs a, const float2* __restrict__ g)
{
    extern __shared__ float2 s_duc[];
    const unsigned tid = threadIdx.x;
    const unsigned I = a.I, L = a.L, P = a.P, IP = a.IP, T = a.T, TS = a.TS, ZS = a.ZS;
    float2* tile = s_duc;             // [IP][TS]
    float2* stage = s_duc + IP * TS;  // [G][ZS]
    const size_t m0 = static_cast<size_t>(blockIdx.x) * T;
    const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned mi = (wave % a.WF) * 64 + (tid & 63); // this lane's frame of the tile
    const unsigned rb0 = wave / a.WF, rb_step = 4 / a.WF, n_rb = IP / R;

    bool first = true;
    for (unsigned k0 = 0; k0 < a.K; k0 += a.G) {
        const unsigned gc = a.K - k0 < a.G ? a.K - k0 : a.G;
        for (unsigned p0 = 0; p0 < P; p0 += a.Pc) {
            const unsigned pc = P - p0 < a.Pc ? P - p0 : a.Pc;
            const unsigned S = T + pc - 1;
            // stage item s of a row: frame fb + s of this call (negative: the handle's history); frame m0 + n takes
            // tap phase p from item n + (p0 + pc - 1 - p)
            const long long fb = static_cast<long long>(m0) - (p0 + pc - 1);
            if (!first) __syncthreads(); // the previous stage has been read
            for (unsigned kk = 0; kk < gc; ++kk) {
                const unsigned k = k0 + kk;
                const uint32_t wk = a.w[k];
                for (unsigned s = tid; s < S; s += kNt) {
                    const long long fr = fb + s;
                    float2 v = {0.0f, 0.0f};
                    if (fr < 0)
                        v = a.hist[static_cast<size_t>(k) * (P - 1) + static_cast<size_t>(fr + (P - 1))];
                    else if (static_cast<size_t>(fr) < a.n_in)
                        v = a.in[static_cast<size_t>(k) * a.in_stride + static_cast<size_t>(fr)];
                    const uint32_t phi = wk * (a.pos + static_cast<uint32_t>(fr) * I);
                    double sn, cs;
                    sincospi(static_cast<double>(phi) * (1.0 / 2147483648.0), &sn, &cs); // the argument is exact
                    float2 z = {0.0f, 0.0f};
                    cmac(z, float2{static_cast<float>(cs), static_cast<float>(sn)}, v);
                    stage[kk * ZS + s] = z;
                }
            }
            __syncthreads();
            if (mi < T) {
                for (unsigned rb = rb0; rb < n_rb; rb += rb_step) {
                    const unsigned r0 = rb * R;
                    const unsigned r_last = (r0 + R < I ? r0 + R : I) - 1;
                    // phases p < p_all have a tap for every phase of the block, phase p_all for some or none
                    const unsigned p_all = L > r_last ? (L - 1 - r_last) / I + 1 : 0;
                    const unsigned p_end = p_all < p0 + pc ? p_all : p0 + pc;
                    float2 acc[R];
#pragma unroll
                    for (int rr = 0; rr < R; ++rr) acc[rr] = first ? float2{0.0f, 0.0f} : tile[(r0 + rr) * TS + mi];
                    for (unsigned kk = 0; kk < gc; ++kk) {
                        const float2* __restrict__ gk = g + static_cast<size_t>(k0 + kk) * P * IP + r0;
                        const float2* zp = stage + kk * ZS + mi + (pc - 1);
#pragma unroll 2
                        for (unsigned p = p0; p < p_end; ++p) {
                            const TapBlock<R> tb = *reinterpret_cast<const TapBlock<R>*>(gk + static_cast<size_t>(p) * IP);
                            const float2 z = zp[-static_cast<int>(p - p0)];
#pragma unroll
                            for (int rr = 0; rr < R; ++rr) cmac(acc[rr], tb.v[rr], z);
                        }
                        if (p_all >= p0 && p_all < p0 + pc) { // p_all < P: the prototype ends inside this phase
                            const TapBlock<R> tb = *reinterpret_cast<const TapBlock<R>*>(gk + static_cast<size_t>(p_all) * IP);
                            const float2 z = zp[-static_cast<int>(p_all - p0)];
#pragma unroll
                            for (int rr = 0; rr < R; ++rr)
                                if (p_all * I + r0 + rr < L && r0 + rr < I) cmac(acc[rr], tb.v[rr], z);
                        }
                    }
#pragma unroll
                    for (int rr = 0; rr < R; ++rr) tile[(r0 + rr) * TS + mi] = acc[rr];
                }
            }
            first = false;
        }
    }
    __syncthreads();

    // sample j of the tile: frame j div I, phase j mod I, at tile[phase][frame]
    const size_t j0 = m0 * I;
    const unsigned n = static_cast<unsigned>(a.n_out - j0 < static_cast<size_t>(T) * I ? a.n_out - j0 : static_cast<size_t>(T) * I);
    float2* __restrict__ out = a.out + j0;
    auto sample = [&](unsigned j) {
        const unsigned m = I == 1 ? j : __umulhi(j, a.rcpI);
        return tile[(j - m * I) * TS + m];
    };
    if (a.vec) { // j0 is even (T I is), so out + j0 keeps the alignment of out
        for (unsigned j = 2 * tid; j < n; j += 2 * kNt) {
            if (j + 1 < n) {
                const float2 lo = sample(j), hi = sample(j + 1);
                *reinterpret_cast<float4*>(out + j) = float4{lo.x, lo.y, hi.x, hi.y};
            } else {
                out[j] = sample(j);
            }
        }
    } else {
        for (unsigned j = tid; j < n; j += kNt) out[j] = sample(j);
    }
}

template <int R>
void launch_r(dim3 grid, size_t smem, hipStream_t s, const DucArgs& a, const float2* g)
{
    hipLaunchKernelGGL(k_duc<R>, grid, dim3(kNt), smem, s, a, g);
}

gr4pm_status design_taps(size_t I, size_t P, double passband, double stopband, std::vector<double>& h)
{
    using gr4pm::set_error;
    if (I < 1 || I > kMaxI) {
        set_error("duc: the interpolation must be in [1, %zu], not %zu", kMaxI, I);
        return GR4PM_ERR_INVALID;
    }
    if (P < 1 || P * I > kMaxL) {
        set_error("duc: %zu taps per phase at an interpolation of %zu: the prototype has 1 .. %zu taps", P, I, kMaxL);
        return GR4PM_ERR_INVALID;
    }
    if (!gr4pm::band_edges_valid(passband, stopband, I, true)) {
        set_error("duc: need 0 <= passband < stopband (units of the input rate) and a cutoff of at most fs / 2");
        return GR4PM_ERR_INVALID;
    }
    gr4pm::kaiser_lowpass(P * I, I, passband, stopband, h, static_cast<double>(I));
    return GR4PM_OK;
}

} // namespace

struct gr4pm_duc {
    size_t K = 0, I = 0, L = 0, P = 0, max_items = 0;
    unsigned R = 0, IP = 0, T = 0, TS = 0, WF = 0, G = 0, Pc = 0, ZS = 0, rcpI = 0;
    size_t smem = 0;
    uint64_t start_index = 0;
    uint64_t pos = 0;       // absolute index of the next output sample
    gr4pm::StreamTail tail; // P - 1 items of every row, frames of one item: nothing is ever carried
    hipStream_t stream = nullptr;
    std::vector<uint32_t> words;
    gr4pm::DevBuf<float2> d_g;
    gr4pm::DevBuf<uint32_t> d_w;
};

using namespace gr4pm;

extern "C" {

gr4pm_status gr4pm_duc_taps(size_t interpolation, size_t taps_per_phase, double passband, double stopband, float* out)
try {
    if (!out) return GR4PM_ERR_INVALID;
    std::vector<double> h;
    GR4PM_TRY(design_taps(interpolation, taps_per_phase, passband, stopband, h));
    round_taps(h, out);
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_duc_create(const gr4pm_duc_params* p, gr4pm_duc** out)
try {
    if (!p || !out) return GR4PM_ERR_INVALID;
    *out = nullptr;
    const size_t K = p->n_channels, I = p->interpolation;
    std::vector<uint32_t> words;
    GR4PM_TRY(frequency_words("duc", p->frequencies, K, kMaxK, words));
    if (I < 1 || I > kMaxI) {
        set_error("duc: the interpolation must be in [1, %zu], not %zu", kMaxI, I);
        return GR4PM_ERR_INVALID;
    }
    for (size_t k = 0; p->gains && k < K; ++k)
        if (!std::isfinite(p->gains[k])) {
            set_error("duc: gains[%zu] is not finite", k);
            return GR4PM_ERR_INVALID;
        }
    if (p->max_items == 0 || p->max_items > (size_t(1) << 31)) {
        set_error("duc: max_items must be in [1, 2^31]");
        return GR4PM_ERR_INVALID;
    }
    if (p->taps && (p->n_taps < 1 || p->n_taps > kMaxL)) {
        set_error("duc: the prototype has 1 .. %zu taps, not %zu", kMaxL, p->n_taps);
        return GR4PM_ERR_INVALID;
    }
    std::vector<float> taps;
    GR4PM_TRY(taps_or_design(p->taps, p->n_taps, [&](std::vector<double>& hd) { return design_taps(I, 12, 0.25, 0.75, hd); }, taps));
    const size_t L = taps.size(), P = (L + I - 1) / I;
    GR4PM_TRY(require_device());
    std::unique_ptr<gr4pm_duc> h(new (std::nothrow) gr4pm_duc);
    if (!h) return GR4PM_ERR_NOMEM;
    h->K = K;
    h->I = I;
    h->L = L;
    h->P = P;
    h->max_items = p->max_items;
    h->start_index = h->pos = p->start_index;
    h->stream = static_cast<hipStream_t>(p->stream);
    // the tile: R phases per lane, T frames (even unless I = 1, so that T I is even) of about kTileItems samples in all;
    // the stage: whole channels while T + P - 1 items of each fit, else one channel and chunks of the p loop
    const size_t R = I >= 8 ? 8 : I >= 4 ? 4 : I >= 2 ? 2 : 1;
    const size_t IP = (I + R - 1) / R * R;
    size_t T = kTileItems / I & ~size_t(1);
    T = T > static_cast<size_t>(kNt) ? static_cast<size_t>(kNt) : T < 2 ? 2 : T;
    size_t G = 1, Pc = P;
    if (T + P - 1 <= kStageItems) {
        G = kStageItems / (T + P - 1);
        if (G > K) G = K;
    } else {
        Pc = kStageItems - T + 1;
    }
    h->R = static_cast<unsigned>(R);
    h->IP = static_cast<unsigned>(IP);
    h->T = static_cast<unsigned>(T);
    h->TS = static_cast<unsigned>(T | 1);
    h->WF = T <= 64 ? 1u : T <= 128 ? 2u : 4u;
    h->G = static_cast<unsigned>(G);
    h->Pc = static_cast<unsigned>(Pc);
    h->ZS = static_cast<unsigned>(T + Pc - 1);
    h->rcpI = reciprocal_word(I);
    h->smem = (IP * h->TS + G * h->ZS) * sizeof(float2); // at most 29 KiB + 16 KiB

    h->words = std::move(words);
    std::vector<float2> g(K * P * IP, float2{0.0f, 0.0f});
    for (size_t k = 0; k < K; ++k) {
        const uint32_t w = h->words[k];
        const double a = p->gains ? p->gains[k] : 1.0;
        for (size_t t = 0; t < L; ++t)
            g[(k * P + t / I) * IP + t % I] = rotated_tap(a * static_cast<double>(taps[t]), w * static_cast<uint32_t>(t));
    }
    GR4PM_TRY(h->d_g.alloc(g.size()));
    GR4PM_TRY(h->d_w.alloc(K));
    GR4PM_TRY(h->tail.alloc(P - 1, 1, K, h->stream));
    GR4PM_TRY(h->d_g.upload(g.data(), g.size(), h->stream));
    GR4PM_TRY(h->d_w.upload(h->words.data(), K, h->stream));
    return finish_create(h, out, "duc");
}
GR4PM_ABI_CATCH

void gr4pm_duc_destroy(gr4pm_duc* h)
try {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    delete h;
}
GR4PM_ABI_CATCH_VOID

gr4pm_status gr4pm_duc_reset(gr4pm_duc* h)
try {
    if (!h) return GR4PM_ERR_INVALID;
    GR4PM_TRY(h->tail.reset(h->stream));
    h->pos = h->start_index;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_duc_output_items(const gr4pm_duc* h, size_t n_in, size_t* n_out)
try {
    if (!h || !n_out) return GR4PM_ERR_INVALID;
    *n_out = n_in * h->I;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_duc_frequencies(const gr4pm_duc* h, double* out)
try {
    if (!h || !out) return GR4PM_ERR_INVALID;
    for (size_t k = 0; k < h->K; ++k) out[k] = folded_frequency(h->words[k]);
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_duc_process(gr4pm_duc* h, const gr4pm_c64* in, size_t in_stride, size_t n_in, gr4pm_c64* out, size_t out_cap,
                               size_t* n_out)
try {
    if (!h || !n_out) return GR4PM_ERR_INVALID;
    *n_out = 0;
    if (n_in > h->max_items) {
        set_error("duc: %zu items per row, the handle was made for %zu", n_in, h->max_items);
        return GR4PM_ERR_OVERFLOW;
    }
    if (n_in == 0) return GR4PM_OK;
    const size_t N = n_in * h->I;
    if (N > out_cap) {
        set_error("duc: %zu samples, room for %zu", N, out_cap);
        return GR4PM_ERR_OVERFLOW;
    }
    if (!in || !out || (h->K > 1 && in_stride < n_in)) {
        set_error("duc: no input or output array, or a row stride of %zu items for %zu items", in_stride, n_in);
        return GR4PM_ERR_INVALID;
    }
    const StreamTail::Plan t = h->tail.plan(n_in);
    DucArgs a;
    a.hist = t.hist;
    a.in = reinterpret_cast<const float2*>(in);
    a.out = reinterpret_cast<float2*>(out);
    a.w = h->d_w.p;
    a.in_stride = in_stride;
    a.n_in = n_in;
    a.n_out = N;
    a.pos = static_cast<uint32_t>(h->pos);
    a.K = static_cast<unsigned>(h->K);
    a.I = static_cast<unsigned>(h->I);
    a.L = static_cast<unsigned>(h->L);
    a.P = static_cast<unsigned>(h->P);
    a.IP = h->IP;
    a.T = h->T;
    a.TS = h->TS;
    a.WF = h->WF;
    a.G = h->G;
    a.Pc = h->Pc;
    a.ZS = h->ZS;
    a.rcpI = h->rcpI;
    a.vec = reinterpret_cast<uintptr_t>(out) % 16 == 0;
    const dim3 grid(static_cast<unsigned>((n_in + h->T - 1) / h->T));
    switch (h->R) {
    case 1: launch_r<1>(grid, h->smem, h->stream, a, h->d_g.p); break;
    case 2: launch_r<2>(grid, h->smem, h->stream, a, h->d_g.p); break;
    case 4: launch_r<4>(grid, h->smem, h->stream, a, h->d_g.p); break;
    default: launch_r<8>(grid, h->smem, h->stream, a, h->d_g.p); break;
    }
    h->tail.launch_history<iq::kC64>(t, in, in_stride, n_in, 0.0f, h->stream);
    GR4PM_HIP_TRY(hipGetLastError());
    h->tail.commit(t);
    h->pos += N;
    *n_out = N;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

} // extern "C"
