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
// history buffer.  The tile's sizes are hostlogic/xlate_geometry.hpp's duc_geometry(): the handle keeps them in a
// prefilled DucArgs, and a call writes only what changes from call to call.
//
// Rational resampling by I / D (gr4pm_duc_create_rational): output sample j of the handle has the
// upsampled index u = j D, the newest item m = u div I and the polyphase branch r = u mod I.  j and m - p are no longer
// an integer apart, so there is no rotator per input item: filter first, then mix.
//     g_k[t] = fl(a_k h[t])                               (host: the product in double, rounded to float once; real)
//     b_k[j] = sum_{p : p I + r < L} g_k[p I + r] v_k[m - p]   (from zero, p ascending, two fmaf per step)
//     q_k(i) = A_k[i div B] (x) T_k[i mod B],  B = 2^10, i the ABSOLUTE output index:  A from double sincospi of the exact
//              phase of the aligned block's first sample (device, once per channel and block, rounded to float),
//              T_k[0 .. B) a host table of freq_xlate.hpp's phasors, the product four fmaf from zero
//     x[i] = sum_k q_k(i) b_k[j]                          (one accumulator from zero, k ascending, cmac)
// k_duc_rational: a workgroup owns I T consecutive samples: since gcd(I, D) = 1 exactly T of every branch.  The about
//   T D + P items per row the tile spans go to LDS once, in ddc.hip's layout (item n at row n mod D, column n div D, odd
//   row length), so that lanes D items apart read consecutive items of a row.  A wave takes 64 samples of one branch at
//   a time: sample q + I l of the tile for lane l, where q < I names the branch ((b0 + q D) mod I); the branch's taps are
//   wave-uniform, a table [k][branch][p] read through the constant address space (scalar loads).  Channels run in groups
//   that fit the stage, one after the other; the accumulators rest in an LDS tile [q][l] with an odd row stride between
//   groups, and the same tile transposes the stride-I results so that the block leaves as 16-byte stores.
// A sample is a function of (absolute output index, the rows' streams) only.  The tile is rduc_geometry()'s, the
// position hostlogic/resample_position.hpp's with lead = 0: 64-bit integers on the host, by value to the kernel.
// Both creates are one create(): gr4pm_duc_create's is the ratio I / 1.
//
// Integer output (gr4pm_duc_process_iq): both kernels are templated on the output format and pack
// a sample where the tile leaves (freq_xlate.hpp's store_tile_iq: iq_format.hpp's pack_item on the two samples a lane
// would have stored, one 8- or 4-byte store); everything in front of the store is the complex64 kernel's, and the
// handle's state stays complex64.  The clipped components are counted per lane, summed per workgroup and added with one
// atomic.  The complex64 instantiations take an empty iq::Out behind their arguments and compile to what they were.
#include "freq_xlate.hpp"
#include "hostlogic/resample_position.hpp"
#include "kaiser_design.hpp"
#include "stream_tail.hpp"

#include <cmath>

namespace {

using namespace gr4pm::hostlogic;
using gr4pm::cmac;
using gr4pm::ConstTaps;
namespace iq = gr4pm::iq;

constexpr size_t kMaxK = 64, kMaxI = 1024, kMaxD = 64, kMaxL = 8192;

struct DucArgs {
    const float2* hist;  // [K][P - 1]: the items in front of in[k][0]
    const float2* in;    // row k at in + k in_stride
    float2* out;         // of an integer format: its items, aligned to the item only
    const uint32_t* w;   // [K] frequency words
    size_t in_stride, n_in, n_out;
    uint32_t pos;        // absolute index of this call's first output sample: the low 32 bits are all the phase needs
    unsigned K, I, L, P;
    DucTile tile;
    unsigned vec;        // out is 16-byte aligned: the tile leaves two samples per store
};

template <int R>
struct TapBlock {
    float2 v[R];
};

template <int R, int F>
__global__ __launch_bounds__(kNt) void k_duc(DucArgs a, const float2* __restrict__ g, iq::Out<F> q)
{
    extern __shared__ float2 s_duc[];
    const unsigned tid = threadIdx.x;
    const unsigned I = a.I, L = a.L, P = a.P, IP = a.tile.IP, T = a.tile.T, TS = a.tile.TS, ZS = a.tile.ZS;
    float2* tile = s_duc;             // [IP][TS]
    float2* stage = s_duc + IP * TS;  // [G][ZS]
    const size_t m0 = static_cast<size_t>(blockIdx.x) * T;
    const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned mi = (wave % a.tile.WF) * 64 + (tid & 63); // this lane's frame of the tile
    const unsigned rb0 = wave / a.tile.WF, rb_step = 4 / a.tile.WF, n_rb = IP / R;

    bool first = true;
    for (unsigned k0 = 0; k0 < a.K; k0 += a.tile.G) {
        const unsigned gc = a.K - k0 < a.tile.G ? a.K - k0 : a.tile.G;
        for (unsigned p0 = 0; p0 < P; p0 += a.tile.Pc) {
            const unsigned pc = P - p0 < a.tile.Pc ? P - p0 : a.tile.Pc;
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
                    float2 z = {0.0f, 0.0f};
                    cmac(z, gr4pm::mixer<1>(wk, a.pos + static_cast<uint32_t>(fr) * I), v);
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
        const unsigned m = I == 1 ? j : __umulhi(j, a.tile.rcpI);
        return tile[(j - m * I) * TS + m];
    };
    if constexpr (F != iq::kC64) { // a.out counts items of F: the tile is packed on its way out, a.vec is not looked at
        unsigned clip = 0;
        gr4pm::store_tile_iq<F>(reinterpret_cast<unsigned char*>(a.out) + j0 * iq::Fmt<F>::item_bytes, n, q.gain, clip, sample);
        // the stage (at least T + Pc - 1 >= 2 items) was last read in front of the barrier above
        iq::add_clipped<kNt / 64>(clip, q.clipped, reinterpret_cast<unsigned*>(stage));
    } else if (a.vec) { // j0 is even (T I is), so out + j0 keeps the alignment of out
        gr4pm::store_tile(out, n, 0, sample);
    } else {
        for (unsigned j = tid; j < n; j += kNt) out[j] = sample(j);
    }
}

struct RducArgs {
    const float2* hist;  // [K][P - 1]: the items in front of in[k][0]
    const float2* in;    // row k at in + k in_stride
    float2* out;         // of an integer format: its items, aligned to the item only
    const uint32_t* w;   // [K] frequency words
    size_t in_stride;
    size_t total;        // P - 1 + n_in: items of a row's virtual stream hist ++ in
    size_t n_out;
    uint64_t u0;         // the call's first sample: its upsampled index, counted from that of in[k][0]
    uint32_t pos;        // absolute index of the call's first sample: the low 32 bits are all the phase needs
    unsigned K, I, D, L, P;
    RducTile tile;
};

// taps: [K][I][P] real taps g_k[p I + r] at [k][r][p], zero where p I + r >= L.  rot: [K][kRotBlock] phasors T_k.
// Both are written at create only and are parameters of their own.
template <int F>
__global__ __launch_bounds__(kNt) void k_duc_rational(RducArgs a, const float* __restrict__ taps, const float2* __restrict__ rot,
                                                      iq::Out<F> q)
{
    extern __shared__ float2 s_rduc[];
    const unsigned tid = threadIdx.x, lane = tid & 63;
    const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned I = a.I, D = a.D, L = a.L, P = a.P, T = a.tile.T, TS = a.tile.TS, RS = a.tile.RS;
    const unsigned IT = I * T, row_items = D * RS;
    float2* tile = s_rduc;                     // [I][TS]
    float2* blk = s_rduc + I * TS;             // [G][kRotSpan]: A_k of the aligned blocks the tile touches
    float2* stage = blk + a.tile.G * kRotSpan; // [G][D][RS]
    const size_t n0 = static_cast<size_t>(blockIdx.x) * IT; // the tile's first sample
    const unsigned n = static_cast<unsigned>(a.n_out - n0 < IT ? a.n_out - n0 : IT);
    const uint64_t u0 = a.u0 + static_cast<uint64_t>(n0) * D;
    const uint64_t c0 = u0 / I;                              // its newest item, counted from in[k][0] ...
    const unsigned b0 = static_cast<unsigned>(u0 - c0 * I); // ... and its branch
    const uint32_t i0 = a.pos + static_cast<uint32_t>(n0);
    const unsigned o0 = i0 & (kRotBlock - 1);
    const unsigned n_blk = (o0 + n - 1) / kRotBlock + 1;     // at most kRotSpan: I T <= 2048
    const unsigned n_units = I * a.tile.chunks;
    auto div_I = [&](unsigned j) { return I == 1 ? j : __umulhi(j, a.tile.rcpI); };
    auto div_D = [&](unsigned j) { return D == 1 ? j : __umulhi(j, a.tile.rcpD); };

    bool first = true;
    for (unsigned k0 = 0; k0 < a.K; k0 += a.tile.G) {
        const unsigned gc = a.K - k0 < a.tile.G ? a.K - k0 : a.tile.G;
        if (!first) __syncthreads(); // the previous group's stage has been read
        // stage item s of a row: item c0 + s of its virtual stream, that is item c0 - (P - 1) + s of this call; the
        // tile's last sample takes its tap 0 from item (b0 + (I T - 1) D) div I + P - 1 < S
        for (unsigned kk = 0; kk < gc; ++kk) {
            const float2* hist = a.hist + static_cast<size_t>(k0 + kk) * (P - 1);
            const float2* in = a.in + static_cast<size_t>(k0 + kk) * a.in_stride;
            gr4pm::stage_by_phase(stage + kk * row_items, a.tile.S, D, a.tile.rcpD, RS, static_cast<size_t>(c0), a.total, hist, P - 1, in);
        }
        if (tid < gc * n_blk) {
            const unsigned kk = tid / n_blk, bb = tid - kk * n_blk;
            blk[kk * kRotSpan + bb] = gr4pm::mixer<1>(a.w[k0 + kk], i0 - o0 + bb * kRotBlock);
        }
        __syncthreads();
        for (unsigned u = wave; u < n_units; u += kNt / 64) {
            // 64 samples of the branch named q: sample q + I l of the tile for l = 64 chunk + lane
            const unsigned chunk = div_I(u), q = u - chunk * I;
            const unsigned ub = b0 + q * D;
            const unsigned e = div_I(ub), r = ub - e * I;   // the first one's newest item, counted from c0; the branch
            const unsigned n_taps = r < L ? div_I(L - r + I - 1) : 0; // taps of h[r::I]
            const unsigned l = chunk * 64 + lane, t = q + I * l;
            if (l < T && t < n) {
                float2 acc = first ? float2{0.0f, 0.0f} : tile[q * TS + l];
                const unsigned ti = o0 + t;
                for (unsigned kk = 0; kk < gc; ++kk) {
                    const ConstTaps g = (ConstTaps)(taps + (static_cast<size_t>(k0 + kk) * I + r) * P);
                    const float2* sk = stage + kk * row_items;
                    float2 b = {0.0f, 0.0f};
                    // tap p takes stage item e + P - 1 - p + l D: row (e + P - 1 - p) mod D, lanes on consecutive columns
                    unsigned col = div_D(e + P - 1), row = (e + P - 1) - col * D, left = n_taps, p = 0;
                    while (left) {
                        const unsigned run = row + 1 < left ? row + 1 : left;
                        const float2* sp = sk + row * RS + col + l;
#pragma unroll 4
                        for (unsigned i = 0; i < run; ++i, sp -= RS, ++p) {
                            const float2 x = *sp;
                            const float gp = g[p];
                            b.x = fmaf(gp, x.x, b.x);
                            b.y = fmaf(gp, x.y, b.y);
                        }
                        left -= run;
                        --col;
                        row = D - 1;
                    }
                    float2 qk = {0.0f, 0.0f};
                    cmac(qk, blk[kk * kRotSpan + ti / kRotBlock], rot[static_cast<size_t>(k0 + kk) * kRotBlock + (ti & (kRotBlock - 1))]);
                    cmac(acc, qk, b);
                }
                tile[q * TS + l] = acc;
            }
        }
        first = false;
    }
    __syncthreads();

    // sample t of the tile is at tile[t mod I][t div I]; one sample alone where out + n0 is only 8-byte aligned
    auto sample = [&](unsigned t) {
        const unsigned l = div_I(t);
        return tile[(t - l * I) * TS + l];
    };
    if constexpr (F != iq::kC64) { // a.out counts items of F
        unsigned clip = 0;
        gr4pm::store_tile_iq<F>(reinterpret_cast<unsigned char*>(a.out) + n0 * iq::Fmt<F>::item_bytes, n, q.gain, clip, sample);
        static_assert(kRotSpan * sizeof(float2) >= kNt / 64 * sizeof(unsigned), "the waves' counts rest in the first group's blocks");
        iq::add_clipped<kNt / 64>(clip, q.clipped, reinterpret_cast<unsigned*>(blk)); // last read in front of the barrier above
    } else {
        float2* __restrict__ out = a.out + n0;
        gr4pm::store_tile(out, n, static_cast<unsigned>(reinterpret_cast<uintptr_t>(out) >> 3) & 1u, sample);
    }
}

// the two designs share their sizes' checks only; their band edges differ: the integer Duc admits passband + stopband
// <= I of the input rate (band_edges_valid: a cutoff within fs / 2), the rational one at most min(1, I / D)
gr4pm_status design_rational_taps(size_t I, size_t D, size_t P, double passband, double stopband, std::vector<double>& h)
{
    GR4PM_TRY(gr4pm::design_sizes("duc", I, kMaxI, D, kMaxD, P, I, "an interpolation", kMaxL));
    // the cutoff, (passband + stopband) / 2 of the input rate, within half of the input rate and half of the output rate
    const double most = I < D ? static_cast<double>(I) / static_cast<double>(D) : 1.0;
    if (!(passband >= 0.0 && passband < stopband && passband + stopband <= most)) {
        gr4pm::set_error("duc: need 0 <= passband < stopband (units of the input rate, the output's is %zu / %zu of it) and a cutoff "
                         "of at most half of the lower of the input and the output rate: passband + stopband <= %g", I, D, most);
        return GR4PM_ERR_INVALID;
    }
    gr4pm::kaiser_lowpass(P * I, I, passband, stopband, h, static_cast<double>(I));
    return GR4PM_OK;
}

gr4pm_status design_taps(size_t I, size_t P, double passband, double stopband, std::vector<double>& h)
{
    GR4PM_TRY(gr4pm::design_sizes("duc", I, kMaxI, 1, kMaxD, P, I, "an interpolation", kMaxL));
    if (!gr4pm::band_edges_valid(passband, stopband, I, true)) {
        gr4pm::set_error("duc: need 0 <= passband < stopband (units of the input rate) and a cutoff of at most fs / 2");
        return GR4PM_ERR_INVALID;
    }
    gr4pm::kaiser_lowpass(P * I, I, passband, stopband, h, static_cast<double>(I));
    return GR4PM_OK;
}

} // namespace

struct gr4pm_duc {
    size_t K = 0, I = 0, D = 1, max_items = 0;
    uint64_t start_index = 0;
    uint64_t pos = 0;       // absolute index of the next output sample
    gr4pm::StreamTail tail; // P - 1 items of every row, frames of one item: nothing is ever carried
    hipStream_t stream = nullptr;
    std::vector<uint32_t> words;
    gr4pm::DevBuf<uint32_t> d_w;
    // what does not change from call to call, in the struct the handle's kernel takes
    DucArgs args = {};   // D = 1
    RducArgs rargs = {}; // D > 1
    unsigned smem = 0, R = 0;         // of a launch
    gr4pm::DevBuf<float2> d_g;        // D = 1: the rotated taps [K][P][IP]
    gr4pm::hostlogic::ResamplePosition at; // D > 1: items taken, the next sample's newest item and branch
    gr4pm::DevBuf<float> d_taps;      // D > 1: [K][I][P]
    gr4pm::DevBuf<float2> d_rot;      // D > 1: [K][kRotBlock]
};

using namespace gr4pm;

// the handle's kernel for the output format F
template <int F>
static void launch(const gr4pm_duc& h, dim3 grid, const DucArgs& a, iq::Out<F> q)
{
    switch (h.R) {
    case 1: hipLaunchKernelGGL((k_duc<1, F>), grid, dim3(kNt), h.smem, h.stream, a, h.d_g.p, q); break;
    case 2: hipLaunchKernelGGL((k_duc<2, F>), grid, dim3(kNt), h.smem, h.stream, a, h.d_g.p, q); break;
    case 4: hipLaunchKernelGGL((k_duc<4, F>), grid, dim3(kNt), h.smem, h.stream, a, h.d_g.p, q); break;
    default: hipLaunchKernelGGL((k_duc<8, F>), grid, dim3(kNt), h.smem, h.stream, a, h.d_g.p, q); break;
    }
}

template <int F>
static void launch(const gr4pm_duc& h, dim3 grid, const RducArgs& a, iq::Out<F> q)
{
    hipLaunchKernelGGL(k_duc_rational<F>, grid, dim3(kNt), h.smem, h.stream, a, h.d_taps.p, h.d_rot.p, q);
}

// either argument struct to the handle's kernel, in the format of the call
template <typename Args>
static void launch_format(const gr4pm_duc& h, dim3 grid, const Args& a, int format, float gain, unsigned long long* clipped)
{
    switch (format) {
    case GR4PM_IQ_SC16: launch(h, grid, a, iq::Out<GR4PM_IQ_SC16>{gain, clipped}); break;
    case GR4PM_IQ_SC8: launch(h, grid, a, iq::Out<GR4PM_IQ_SC8>{gain, clipped}); break;
    case GR4PM_IQ_CU8: launch(h, grid, a, iq::Out<GR4PM_IQ_CU8>{gain, clipped}); break;
    default: launch(h, grid, a, iq::Out<iq::kC64>{}); break;
    }
}

// both creates: gr4pm_duc_create's handle is the ratio I / 1
static gr4pm_status create(const gr4pm_duc_rational_params* p, gr4pm_duc** out)
{
    const size_t K = p->n_channels, I = p->interpolation, D = p->decimation;
    std::vector<uint32_t> words;
    GR4PM_TRY(frequency_words("duc", p->frequencies, K, kMaxK, words));
    GR4PM_TRY(resample_ratio("duc", I, kMaxI, D, kMaxD));
    GR4PM_TRY(finite_gains("duc", p->gains, K));
    GR4PM_TRY(per_call_cap("duc", "max_items", p->max_items));
    GR4PM_TRY(prototype_length("duc", p->taps, p->n_taps, kMaxL));
    std::vector<float> taps;
    GR4PM_TRY(taps_or_design(p->taps, p->n_taps, [&](std::vector<double>& hd) {
        return D > 1 ? design_rational_taps(I, D, 12, 0.25, 0.75, hd) : design_taps(I, 12, 0.25, 0.75, hd);
    }, taps));
    const size_t L = taps.size(), P = (L + I - 1) / I;
    GR4PM_TRY(require_device());
    std::unique_ptr<gr4pm_duc> h(new (std::nothrow) gr4pm_duc);
    if (!h) return GR4PM_ERR_NOMEM;
    h->K = K;
    h->I = I;
    h->D = D;
    h->max_items = p->max_items;
    h->start_index = h->pos = p->start_index;
    h->stream = static_cast<hipStream_t>(p->stream);
    h->words = std::move(words);
    GR4PM_TRY(h->d_w.alloc(K));
    const unsigned Ku = static_cast<unsigned>(K), Iu = static_cast<unsigned>(I), Lu = static_cast<unsigned>(L),
                   Pu = static_cast<unsigned>(P);
    if (D > 1) {
        RducArgs& a = h->rargs;
        a.w = h->d_w.p;
        a.K = Ku, a.I = Iu, a.D = static_cast<unsigned>(D), a.L = Lu, a.P = Pu;
        RducGeometry geo;
        if (!rduc_geometry(I, D, L, K, geo)) {
            set_error("duc: no tile of %zu / %zu with %zu taps fits the stage", I, D, L);
            return GR4PM_ERR_INVALID;
        }
        a.tile = geo.tile, h->smem = geo.smem;
        h->at.I = I, h->at.D = D;
        std::vector<float> g(K * I * P, 0.0f);
        std::vector<float2> rot(K * kRotBlock);
        for (size_t k = 0; k < K; ++k) {
            const double gain = p->gains ? p->gains[k] : 1.0;
            for (size_t t = 0; t < L; ++t) g[(k * I + t % I) * P + t / I] = static_cast<float>(gain * static_cast<double>(taps[t]));
            for (size_t t = 0; t < kRotBlock; ++t) rot[k * kRotBlock + t] = rotated_tap(1.0, h->words[k] * static_cast<uint32_t>(t));
        }
        GR4PM_TRY(h->d_taps.alloc(g.size()));
        GR4PM_TRY(h->d_rot.alloc(rot.size()));
        GR4PM_TRY(h->d_taps.upload(g.data(), g.size(), h->stream));
        GR4PM_TRY(h->d_rot.upload(rot.data(), rot.size(), h->stream));
        if (h->smem > 48 * 1024)
            GR4PM_TRY(raise_dynamic_lds({reinterpret_cast<const void*>(&k_duc_rational<iq::kC64>),
                                         reinterpret_cast<const void*>(&k_duc_rational<GR4PM_IQ_SC16>),
                                         reinterpret_cast<const void*>(&k_duc_rational<GR4PM_IQ_SC8>),
                                         reinterpret_cast<const void*>(&k_duc_rational<GR4PM_IQ_CU8>)},
                                        kRducLdsItemsMost * sizeof(float2), "duc"));
    } else {
        DucArgs& a = h->args;
        a.w = h->d_w.p;
        a.K = Ku, a.I = Iu, a.L = Lu, a.P = Pu;
        const DucGeometry geo = duc_geometry(I, L, K);
        a.tile = geo.tile, h->smem = geo.smem, h->R = geo.R;
        const size_t IP = geo.tile.IP;
        std::vector<float2> g(K * P * IP, float2{0.0f, 0.0f});
        for (size_t k = 0; k < K; ++k) {
            const uint32_t w = h->words[k];
            const double gain = p->gains ? p->gains[k] : 1.0;
            for (size_t t = 0; t < L; ++t)
                g[(k * P + t / I) * IP + t % I] = rotated_tap(gain * static_cast<double>(taps[t]), w * static_cast<uint32_t>(t));
        }
        GR4PM_TRY(h->d_g.alloc(g.size()));
        GR4PM_TRY(h->d_g.upload(g.data(), g.size(), h->stream));
    }
    GR4PM_TRY(h->d_w.upload(h->words.data(), K, h->stream));
    GR4PM_TRY(h->tail.alloc(P - 1, 1, K, h->stream));
    return finish_create(h, out, "duc");
}

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
    const gr4pm_duc_rational_params q = {p->n_channels, p->interpolation, p->frequencies, p->gains, p->taps, p->n_taps,
                                         p->max_items, p->start_index, p->stream, 1};
    return create(&q, out);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_duc_rational_taps(size_t interpolation, size_t decimation, size_t taps_per_phase, double passband,
                                     double stopband, float* out)
try {
    if (!out) return GR4PM_ERR_INVALID;
    std::vector<double> h;
    GR4PM_TRY(design_rational_taps(interpolation, decimation, taps_per_phase, passband, stopband, h));
    round_taps(h, out);
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_duc_create_rational(const gr4pm_duc_rational_params* p, gr4pm_duc** out)
try {
    if (!p || !out) return GR4PM_ERR_INVALID;
    *out = nullptr;
    return create(p, out);
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
    h->at.reset();
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_duc_output_items(const gr4pm_duc* h, size_t n_in, size_t* n_out)
try {
    if (!h || !n_out) return GR4PM_ERR_INVALID;
    *n_out = h->D > 1 ? static_cast<size_t>(h->at.samples(n_in)) : n_in * h->I;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_duc_tile_items(const gr4pm_duc* h, size_t* samples)
try {
    if (!h || !samples) return GR4PM_ERR_INVALID;
    *samples = h->I * static_cast<size_t>(h->D > 1 ? h->rargs.tile.T : h->args.tile.T);
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

} // extern "C"

// process() and process_iq(): format iq::kC64 for complex64 samples.  out and out_cap count items of the format
static gr4pm_status process(gr4pm_duc* h, const gr4pm_c64* in, size_t in_stride, size_t n_in, void* out, int format, float gain,
                            size_t out_cap, size_t* n_out, unsigned long long* clipped)
{
    if (n_in > h->max_items) {
        set_error("duc: %zu items per row, the handle was made for %zu", n_in, h->max_items);
        return GR4PM_ERR_OVERFLOW;
    }
    if (n_in == 0) return GR4PM_OK;
    const bool rational = h->D > 1;
    const uint64_t F = rational ? h->at.samples(n_in) : static_cast<uint64_t>(n_in) * h->I;
    const uint64_t tile = static_cast<uint64_t>(h->I) * (rational ? h->rargs.tile.T : h->args.tile.T), blocks = (F + tile - 1) / tile;
    if (F > out_cap || blocks > 0x7FFFFFFFu) {
        set_error("duc: %llu samples, room for %zu", static_cast<unsigned long long>(F), out_cap);
        return GR4PM_ERR_OVERFLOW;
    }
    if (!in || (F && !out) || (h->K > 1 && in_stride < n_in)) {
        set_error("duc: no input or output array, or a row stride of %zu items for %zu items", in_stride, n_in);
        return GR4PM_ERR_INVALID;
    }
    const StreamTail::Plan t = h->tail.plan(n_in);
    // the per-call fields of either argument struct
    auto fill = [&](auto& a) {
        a.hist = t.hist;
        a.in = reinterpret_cast<const float2*>(in);
        a.out = reinterpret_cast<float2*>(out);
        a.in_stride = in_stride;
        a.n_out = static_cast<size_t>(F);
        a.pos = static_cast<uint32_t>(h->pos);
    };
    const dim3 grid(static_cast<unsigned>(blocks));
    if (rational) {
        RducArgs a = h->rargs;
        fill(a);
        a.total = t.H + n_in;
        a.u0 = h->at.first();
        if (F) launch_format(*h, grid, a, format, gain, clipped);
    } else {
        DucArgs a = h->args;
        fill(a);
        a.n_in = n_in;
        a.vec = reinterpret_cast<uintptr_t>(out) % 16 == 0;
        launch_format(*h, grid, a, format, gain, clipped);
    }
    h->tail.launch_history<iq::kC64>(t, in, in_stride, n_in, 0.0f, h->stream);
    GR4PM_HIP_TRY(hipGetLastError());
    h->tail.commit(t);
    if (rational) h->at.advance(n_in, F);
    h->pos += F;
    *n_out = static_cast<size_t>(F);
    return GR4PM_OK;
}

extern "C" {

gr4pm_status gr4pm_duc_process(gr4pm_duc* h, const gr4pm_c64* in, size_t in_stride, size_t n_in, gr4pm_c64* out, size_t out_cap,
                               size_t* n_out)
try {
    if (!h || !n_out) return GR4PM_ERR_INVALID;
    *n_out = 0;
    return process(h, in, in_stride, n_in, out, iq::kC64, 0.0f, out_cap, n_out, nullptr);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_duc_process_iq(gr4pm_duc* h, const gr4pm_c64* in, size_t in_stride, size_t n_in, void* out, int format, float gain,
                                  size_t out_cap, size_t* n_out, unsigned long long* clipped)
try {
    if (!h || !n_out) return GR4PM_ERR_INVALID;
    *n_out = 0;
    if (!iq::valid(format)) {
        set_error("duc: format %d is none of GR4PM_IQ_SC16 / SC8 / CU8", format);
        return GR4PM_ERR_INVALID;
    }
    return process(h, in, in_stride, n_in, out, format, gain == 0.0f ? iq::default_gain(format) : gain, out_cap, n_out, clipped);
}
GR4PM_ABI_CATCH

} // extern "C"
