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
// k_fft_duc_mixed_assemble: one workgroup of four waves per segment, the segment's 2048 bins in LDS, a row's sizes from a
//   descriptor table (k_fft_duc_assemble: the same two bodies with them from the launch, for a bank whose rows are all
//   alike).  The rows go through in groups of four, a wave each: the wave stages the B_k items of its row from
//   the carried items or the input, rotated on the way in (one double sincospi per staged item, four fmaf from zero), and
//   runs log2 B_k radix-2 autosort (Stockham) stages between two LDS buffers of its own, natural order in and out, twiddles
//   exp(-2 pi j m / 512) from a table made in double: section 25's loop with the conjugate twiddles, with wave-level
//   synchronisation only, since no other wave touches the buffers.  Behind one barrier all 256 threads add the group's
//   rows to the bins, one row after the other in ascending k with a barrier between them: thread t takes the table's
//   items t, t + 256, ..., which are different bins (R B <= N), so within a row no two threads meet and across rows the
//   barrier orders them.  Whoever adds to a bin has seen all its earlier rows: no atomics, and the slices may overlap and
//   wrap bin 0.  The bins leave as spec[segment][2048].
// k_fft_duc_inverse: k_fft_ddc_forward's wave on the one-exchange transform of fft2048_w64.hpp, whose input and output
//   layouts are the same (register j of lane l is item / bin l + 64 j).  It reads a spectrum with real and imaginary
//   parts swapped, transforms forward and swaps back: the exact inverse, j conj(F(j conj S)) = F^-1(S) N, with no new
//   transform.  Only the samples p >= V are stored.
// A launch pair covers at most kChunk segments, so the spectra of a call of any length stay within one 64 MiB buffer
// that the next pair reuses in stream order.  No atomics, no scratch; a segment's samples are a function of its B items
// per row, the tables and its index only, whatever the cuts into calls.
// One handle (FftDucBank), one create and one call serve both ABI types.  The MixedFftDuc (DESIGN.md section 28,
// hostlogic/fft_duc_mixed_plan.hpp) gives every row its own I_k, B_k = N / I_k, taps and image count on one segment grid, a_s
// being a multiple of every I_k, and counts a call in slots of Imax output samples; the FftDuc is the bank whose
// interpolations are all equal, built by gr4pm_fft_duc_create from its scalars, where a slot is one item of every row; the
// call picks the assembling kernel by what the bank holds, not by its ABI type.  The rows carry different numbers of items
// between calls, which k_fft_duc_mixed_history moves between two buffers as stream_tail.hpp's kernel does for rows of one
// length.
// Built with FFT_FLAGS: the transforms and the products may contract to FMA.  The rotator is written in explicit fmaf
// (freq_xlate.hpp's cmac), so it is the Duc's under either set of flags.
// Integer output (gr4pm_fft_duc_process_iq / _mixed_process_iq): k_fft_duc_inverse is templated on
// the output format and packs a sample where it stores it, an item per lane.  The kernel is fft_duc_inverse.hpp's: this
// unit instantiates it for complex64, fft_duc_iq.hip for the integer formats, so that this unit's kernels compile as they
// did before there were any.  iq_format.hpp's pack keeps its product and its sum apart under these flags too (cu8's
// x gain + 127.5 would fuse where the gain is no power of two), so the bytes are gr4pm_iq_pack's.
#include "fft_duc_inverse.hpp"
#include "freq_xlate.hpp"
#include "hostlogic/fft_duc_mixed_plan.hpp"

#include <algorithm>
#include <cmath>

namespace {

namespace iq = gr4pm::iq;
using namespace gr4pm;
using gr4pm::hostlogic::fft_duc_mixed_carried_offsets;
using gr4pm::hostlogic::fft_duc_mixed_default_overlap;
using gr4pm::hostlogic::fft_duc_mixed_items;
using gr4pm::hostlogic::fft_duc_mixed_max_interpolation;
using gr4pm::hostlogic::fft_duc_mixed_row;
using gr4pm::hostlogic::fft_duc_mixed_slots_fit;
using gr4pm::hostlogic::fft_duc_mixed_table_offsets;
using gr4pm::hostlogic::fft_duc_mixed_validate;
using gr4pm::hostlogic::fft_duc_mixed_validate_channels;
using gr4pm::hostlogic::FftDucMixedRefusal;
using gr4pm::hostlogic::FftDucMixedRow;
using gr4pm::hostlogic::FftDucMixedVerdict;
using gr4pm::hostlogic::fft_ddc_bin;
using gr4pm::hostlogic::fft_ddc_pow2;
using gr4pm::hostlogic::fft_ddc_table_word;
using gr4pm::hostlogic::fft_duc_item_index;
using gr4pm::hostlogic::fft_duc_plan;
using gr4pm::hostlogic::fft_duc_shape;
using gr4pm::hostlogic::FftDucPlan;
using gr4pm::hostlogic::FftDucShape;
using gr4pm::hostlogic::kFftDucMaxI;
using gr4pm::hostlogic::kFftDucMaxK;
using gr4pm::hostlogic::kFftDucMinHop;
using gr4pm::hostlogic::kFftDucMinI;

constexpr size_t kN = kFftN;
constexpr size_t kChunk = 4096;  // segments of one launch pair: 64 MiB of spectra
constexpr int kTwiddles = 256;   // exp(-2 pi j m / 512), m < 256
constexpr int kAsmWaves = 4, kAsmThreads = kAsmWaves * 64;

// what the lanes of one wave wrote to LDS is visible to its other lanes behind this: no workgroup barrier where a wave
// works in buffers of its own
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One (segment, row) of an assembling kernel, by one wave in two LDS buffers of B items of its own (`mine`): the row's B
// items from item v0 of hist[0 .. H) ++ in on, rotated on the way in, then log2 B Stockham stages.  The result is in
// mine + (logB & 1) B.  Both assembling kernels instantiate this under the unit's one set of flags, so a row goes through
// the same instructions whichever kernel it is in.  Wave-level synchronisation only
__device__ __forceinline__ void fft_duc_row_body(float2* mine, const float2* tw, const float2* hist, size_t H, const float2* in,
                                                 size_t v0, uint32_t wk, uint32_t i0, uint32_t I, uint32_t logB, uint32_t lane)
{
    const uint32_t B = 1u << logB;
    for (uint32_t n = lane; n < B; n += 64) {
        const size_t v = v0 + n;
        const float2 x = v < H ? hist[v] : in[v - H];
        float2 z = {0.0f, 0.0f};
        cmac(z, mixer<1>(wk, i0 + n * I), x);
        mine[n] = z;
    }
    wave_sync();
    // stage of sub-transform length Ns: butterfly j takes items j and j + B / 2, position q = j mod Ns of its
    // sub-transform, and writes items (j - q) 2 + q and Ns later.  Natural order in, natural order out
    for (uint32_t ls = 0; ls < logB; ++ls) {
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

// One row into the segment's bins, by all kAsmThreads threads: thread t takes the table's items t, t + 256, ..., which are
// different bins (R B <= N).  Z: the row's B-point transform, c: its nearest bin
__device__ __forceinline__ void fft_duc_add_body(float2* S, const float2* Z, const float2* __restrict__ Gk, uint32_t c, uint32_t B,
                                                 uint32_t RB, uint32_t tid)
{
    const uint32_t bin0 = c + static_cast<uint32_t>(kN) - RB / 2; // bin of the table's item 0, before the wrap
    for (uint32_t t = tid; t < RB; t += kAsmThreads) {
        const uint32_t b = (bin0 + t) & (kN - 1);
        const float2 g = Gk[t], z = Z[b & (B - 1)];
        float2 s = S[b];
        s.x += g.x * z.x - g.y * z.y;
        s.y += g.x * z.y + g.y * z.x;
        S[b] = s;
    }
}

// a row of the bank, fixed at create
struct MixedRow {
    uint32_t w;        // frequency word
    uint32_t logB;     // log2 B_k
    uint32_t I;        // I_k = N / B_k
    uint32_t R;        // images
    uint32_t g_off;    // the row's table in G
    uint32_t hist_off; // the row's carried items in hist
};

// A bank whose rows all have one I and one R: what the descriptors say is the same for every row, and goes with the launch
// (measured: a uniform K = 64 is 5 % faster this way, and another 0.5 % with the words packed and not 24 bytes apart in
// the descriptors: profiles/fft_duc_bench.txt).  A slot is one item then, the tables are R B items apart and the rows'
// carried items B - 1.
struct AsmArgs {
    const float2* hist;   // row k's H carried items at hist + k (B - 1)
    const float2* in;     // row k at in + k in_stride
    size_t in_stride;
    size_t H;
    size_t seg0;          // the launch's first segment, counted from the call's
    const float2* G;      // [K][R B]: item t is u = t - R B / 2
    const float2* tw;     // [256]
    const uint32_t* w;    // [K] frequency words, packed
    float2* spec;         // [segments of the launch][2048]
    uint32_t index0;      // absolute index of the first input item of the launch's first segment (its low 32 bits)
    uint32_t K, I, logB, R;
    uint32_t hop, hop_items;
};

// blockIdx.x: the segment of the launch; kAsmThreads threads; dynamic LDS: tw[256] | S[2048] | per wave two buffers of B
// items.  The two bodies are k_fft_duc_mixed_assemble's below, so the bits are
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
        if (k < a.K) // uniform over the wave, which works in its own two buffers up to the barrier below
            fft_duc_row_body(mine, tw, a.hist + static_cast<size_t>(k) * (B - 1), a.H, a.in + static_cast<size_t>(k) * a.in_stride, v0,
                             a.w[k], i0, a.I, a.logB, lane);
        __syncthreads();

        // the group's rows into the segment's bins, k ascending; the barrier orders a bin's rows
        const uint32_t gc = a.K - k0 < kAsmWaves ? a.K - k0 : kAsmWaves;
        for (uint32_t kk = 0; kk < gc; ++kk) {
            fft_duc_add_body(S, bufs + (kk * 2 + src) * B, a.G + static_cast<size_t>(k0 + kk) * RB, fft_ddc_bin(a.w[k0 + kk]), B, RB,
                             tid);
            __syncthreads(); // behind the last row: the buffers take the next group
        }
    }

    float2* o = a.spec + static_cast<size_t>(seg) * kN;
    for (uint32_t b = tid; b < kN; b += kAsmThreads) o[b] = S[b];
}

struct MixedAsmArgs {
    const float2* hist;   // row k's H_k carried items at hist + rows[k].hist_off
    const float2* in;     // row k at in + k in_stride
    size_t in_stride;
    size_t seg0;          // the launch's first segment, counted from the call's
    const float2* G;
    const float2* tw;     // [256]
    const MixedRow* rows; // [K]
    float2* spec;         // [segments of the launch][2048]
    uint32_t index0;      // absolute index of the first output sample of the launch's first segment (its low 32 bits)
    uint32_t K, Bmax;
    uint32_t carried;     // V + pending Imax: the output samples the carried items stand for; H_k = carried / I_k
    uint32_t hop;         // hop / I_k items of row k complete a segment
};

// blockIdx.x: the segment of the launch; kAsmThreads threads; dynamic
// LDS: tw[256] | S[2048] | per wave two buffers of Bmax items, of which row k uses the first 2 B_k.  The waves of a group run
// log2 B_k stages each, synchronised per wave; every __syncthreads below is outside the `k < K` branch and inside loops
// whose bounds (K, gc) are the same for all four waves, so all of them reach each one.  H_k and hop / I_k come from the two
// launch constants by a shift, so the table is written once, at create.
__global__ __launch_bounds__(kAsmThreads) void k_fft_duc_mixed_assemble(MixedAsmArgs a)
{
    extern __shared__ float2 s_fft_duc[];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float2* tw = s_fft_duc;
    float2* S = s_fft_duc + kTwiddles;
    float2* bufs = S + kN;
    float2* mine = bufs + wave * 2 * a.Bmax;
    for (uint32_t m = tid; m < kTwiddles; m += kAsmThreads) tw[m] = a.tw[m];
    for (uint32_t b = tid; b < kN; b += kAsmThreads) S[b] = float2{0.0f, 0.0f};
    __syncthreads();

    const uint32_t seg = blockIdx.x;
    const uint32_t i0 = a.index0 + seg * a.hop;

    for (uint32_t k0 = 0; k0 < a.K; k0 += kAsmWaves) {
        const uint32_t k = k0 + wave;
        if (k < a.K) { // uniform over the wave
            const MixedRow r = a.rows[k];
            const uint32_t logI = 11 - r.logB;
            const size_t H = a.carried >> logI;
            const size_t v0 = (a.seg0 + seg) * (a.hop >> logI);
            fft_duc_row_body(mine, tw, a.hist + r.hist_off, H, a.in + static_cast<size_t>(k) * a.in_stride, v0, r.w, i0, r.I, r.logB,
                             lane);
        }
        __syncthreads();

        const uint32_t gc = a.K - k0 < kAsmWaves ? a.K - k0 : kAsmWaves;
        for (uint32_t kk = 0; kk < gc; ++kk) {
            const MixedRow r = a.rows[k0 + kk];
            const uint32_t B = 1u << r.logB;
            fft_duc_add_body(S, bufs + kk * 2 * a.Bmax + (r.logB & 1) * B, a.G + r.g_off, fft_ddc_bin(r.w), B, r.R << r.logB, tid);
            __syncthreads(); // behind the last row: the buffers take the next group
        }
    }

    float2* o = a.spec + static_cast<size_t>(seg) * kN;
    for (uint32_t b = tid; b < kN; b += kAsmThreads) o[b] = S[b];
}

// blockIdx.y: the row.  Its virtual stream is hist[0 .. H_k) ++ in[0 .. n_k) with H_k = carried / I_k, n_k = taken / I_k
// (taken: the call's slots in output samples); the last H_k' = carried_new / I_k items of it go to hist_new
__global__ __launch_bounds__(256) void k_fft_duc_mixed_history(const float2* hist, const float2* in, size_t in_stride,
                                                               const MixedRow* rows, uint32_t carried, size_t taken,
                                                               uint32_t carried_new, float2* hist_new)
{
    const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x, k = blockIdx.y;
    const MixedRow r = rows[k];
    const uint32_t logI = 11 - r.logB;
    const size_t H = carried >> logI, n = taken >> logI, H_new = carried_new >> logI;
    if (i >= H_new) return;
    const size_t v = H + n - H_new + i;
    hist_new[r.hist_off + i] = v < H ? hist[r.hist_off + v] : in[k * in_stride + (v - H)];
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

// The one handle behind both ABI types: K rows with an interpolation each on the segment grid of (Imax, V), counted in
// slots of Imax output samples.  An FftDuc is the bank whose interpolations are all equal: a slot is one item of every row.
struct FftDucBank {
    virtual ~FftDucBank() = default; // the ABI types derive from it and are deleted through it
    const char* name = ""; // of the entry points' messages: fft_duc or fft_duc_mixed
    size_t K = 0, Imax = 0, V = 0, Bmax = 0;
    uint32_t max_ratio = 1; // Imax / min I_k: items per slot of the longest row
    MixedRow alike = {};    // a row's sizes where all rows have one I and one R (logB != 0 then): k_fft_duc_assemble serves
    uint64_t start_index = 0;
    uint64_t taken = 0; // slots since create or reset
    FftDucShape shape = {}; // of Imax: its items are slots
    hipStream_t stream = nullptr;
    size_t max_waves = 2048; // of one inverse launch: eight per compute unit, at most 2048
    std::vector<uint32_t> words;
    std::vector<FftDucMixedRow> rows;
    int cur = 0; // which buffer holds the carried items
    gr4pm::DevBuf<float2> d_hist[2];
    gr4pm::DevBuf<float4> d_tT;
    gr4pm::DevBuf<cf> d_cc, d_spec;
    gr4pm::DevBuf<float2> d_tw, d_G;
    gr4pm::DevBuf<MixedRow> d_rows;
    gr4pm::DevBuf<uint32_t> d_w; // the words again, packed, for k_fft_duc_assemble
};

// what a handle needs for its transforms, whatever its rows: the inverse kernel's tables and wave count, the assembling
// kernel's twiddles and the buffer of spectra.  The host vectors live until the create's wait
struct TransformTables {
    std::vector<float4> tT;
    std::vector<cf> cc;
    std::vector<float2> tw;
};

gr4pm_status transform_tables(FftDucBank& h, TransformTables& t)
{
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
        h.max_waves = std::min(h.max_waves, static_cast<size_t>(prop.multiProcessorCount) * kW64Waves);
    t.tT.resize(kW64TwFloat4);
    t.cc.resize(64);
    build_w64_tables(
        [](int k) {
            const double ang = -2.0 * M_PI * k / kFftN;
            return mk(static_cast<float>(std::cos(ang)), static_cast<float>(std::sin(ang)));
        },
        t.tT.data(), t.cc.data());
    t.tw.resize(kTwiddles);
    for (int m = 0; m < kTwiddles; ++m) {
        double cs, sn;
        unit_phasor(0u - (static_cast<uint32_t>(m) << 23), cs, sn); // -m / 512 of a turn
        t.tw[m] = float2{static_cast<float>(cs), static_cast<float>(sn)};
    }
    GR4PM_TRY(h.d_tT.alloc(t.tT.size()));
    GR4PM_TRY(h.d_cc.alloc(t.cc.size()));
    GR4PM_TRY(h.d_tw.alloc(t.tw.size()));
    GR4PM_TRY(h.d_spec.alloc(kChunk * kN));
    GR4PM_TRY(h.d_tT.upload(t.tT.data(), t.tT.size(), h.stream));
    GR4PM_TRY(h.d_cc.upload(t.cc.data(), t.cc.size(), h.stream));
    GR4PM_TRY(h.d_tw.upload(t.tw.data(), t.tw.size(), h.stream));
    return GR4PM_OK;
}

// the inverse transforms of the `segs` spectra of a launch pair, the call's segments from `done` on
// in the call's format: iq::kC64 for complex64, where gain and clipped are not looked at
void launch_inverse(const FftDucBank& h, InvArgs b, size_t done, size_t segs, int format, float gain, unsigned long long* clipped)
{
    const size_t per_wave = (segs + h.max_waves - 1) / h.max_waves;
    const size_t waves = (segs + per_wave - 1) / per_wave;
    b.seg0 = done, b.n_seg = static_cast<uint32_t>(segs), b.run = static_cast<uint32_t>(per_wave);
    const dim3 grid(static_cast<unsigned>((waves + kW64Waves - 1) / kW64Waves));
    InvArgsIq bi = {};
    static_cast<InvArgs&>(bi) = b;
    bi.gain = gain, bi.clipped = clipped;
    if (format == iq::kC64)
        hipLaunchKernelGGL(k_fft_duc_inverse<iq::kC64>, grid, dim3(kW64Threads), 0, h.stream, b);
    else
        fft_duc_launch_inverse_iq(grid, h.stream, bi, format);
}

// dynamic LDS of both assembling kernels
size_t assemble_lds(size_t Bmax) { return (kTwiddles + kN + kAsmWaves * 2 * Bmax) * sizeof(float2); }

// The create of both handles, behind the fronts' checks of their own arguments: words the K frequency words, gains or
// null, I and R per row, taps[k] row k's prototype or empty for the default design of taps_per_phase I_k taps, overlap < 0
// for the default.  Messages speak of the arrays of gr4pm_fft_duc_mixed_params; the FftDuc's front has refused every
// scalar they could name before it calls this.
gr4pm_status create_bank(FftDucBank& h, const char* name, std::vector<uint32_t> words, const double* gains, const std::vector<size_t>& I,
                         const std::vector<size_t>& R, std::vector<std::vector<float>> taps, size_t taps_per_phase, ptrdiff_t overlap,
                         uint64_t start_index, void* stream)
{
    const size_t K = words.size();
    std::vector<size_t> L(K);
    for (size_t k = 0; k < K; ++k) {
        if (!fft_ddc_pow2(I[k]) || I[k] < kFftDucMinI || I[k] > kFftDucMaxI) {
            set_error("%s: interpolations[%zu] must be a power of two in [%u, %u], not %zu", name, k, kFftDucMinI, kFftDucMaxI, I[k]);
            return GR4PM_ERR_INVALID;
        }
        if (taps[k].empty() && (taps_per_phase < 1 || taps_per_phase * I[k] > kN)) {
            set_error("%s: %zu taps per phase at an interpolation of %zu: the prototype has 1 .. %zu taps", name, taps_per_phase, I[k], kN);
            return GR4PM_ERR_INVALID;
        }
        L[k] = taps[k].empty() ? taps_per_phase * I[k] : taps[k].size();
    }
    const FftDucMixedVerdict sizes = fft_duc_mixed_validate_channels(K, I.data(), R.data(), L.data());
    if (sizes.refusal == FftDucMixedRefusal::images) {
        set_error("%s: images[%zu] must be a power of two in [1, %zu], not %zu", name, sizes.channel, I[sizes.channel], R[sizes.channel]);
        return GR4PM_ERR_INVALID;
    }
    if (sizes.refusal != FftDucMixedRefusal::none) {
        set_error("%s: invalid sizes of row %zu", name, sizes.channel);
        return GR4PM_ERR_INVALID;
    }
    for (size_t k = 0; k < K; ++k) {
        if (taps[k].empty()) {
            taps[k].resize(L[k]);
            GR4PM_TRY(gr4pm_duc_taps(I[k], taps_per_phase, 0.25, 0.75, taps[k].data()));
        }
        for (size_t t = 0; t < L[k]; ++t)
            if (!std::isfinite(taps[k][t])) {
                set_error("%s: taps[%zu] of row %zu is not finite", name, t, k);
                return GR4PM_ERR_INVALID;
            }
    }
    const size_t Imax = fft_duc_mixed_max_interpolation(K, I.data());
    const size_t V = overlap < 0 ? fft_duc_mixed_default_overlap(K, L.data()) : static_cast<size_t>(overlap);
    const FftDucMixedVerdict v = fft_duc_mixed_validate(K, I.data(), R.data(), L.data(), V);
    switch (v.refusal) {
    case FftDucMixedRefusal::none: break;
    case FftDucMixedRefusal::overlap_multiple:
        set_error("%s: the overlap %zu is no multiple of the largest interpolation %zu", name, V, Imax);
        return GR4PM_ERR_INVALID;
    case FftDucMixedRefusal::overlap_low:
        set_error("%s: the overlap %zu is below the reach of row %zu: its %zu taps need %zu", name, V, v.channel, L[v.channel],
                  L[v.channel] - 1);
        return GR4PM_ERR_INVALID;
    case FftDucMixedRefusal::overlap_high:
        set_error("%s: the overlap %zu leaves a hop below %u: at most %zu", name, V, kFftDucMinHop, kN - kFftDucMinHop);
        return GR4PM_ERR_INVALID;
    default: set_error("%s: invalid sizes", name); return GR4PM_ERR_INVALID;
    }
    GR4PM_TRY(require_device());
    h.name = name, h.K = K, h.Imax = Imax, h.V = V;
    h.start_index = start_index;
    h.shape = fft_duc_shape(static_cast<uint32_t>(Imax), static_cast<uint32_t>(V));
    h.stream = static_cast<hipStream_t>(stream);
    h.words = std::move(words);
    TransformTables tables;
    GR4PM_TRY(transform_tables(h, tables));
    std::vector<size_t> g_off(K), hist_off(K);
    std::vector<float2> G(fft_duc_mixed_table_offsets(K, I.data(), R.data(), g_off.data()));
    const size_t hist_items = fft_duc_mixed_carried_offsets(K, I.data(), hist_off.data());
    std::vector<MixedRow> rows(K);
    h.rows.resize(K);
    for (size_t k = 0; k < K; ++k) {
        const uint32_t w = h.words[k], c = fft_ddc_bin(w);
        const double gain = gains ? gains[k] : 1.0;
        const size_t B = kN / I[k], RB = R[k] * B;
        for (size_t t = 0; t < RB; ++t)
            G[g_off[k] + t] = response(taps[k], gain, w, c, static_cast<int32_t>(t) - static_cast<int32_t>(RB / 2));
        h.rows[k] = fft_duc_mixed_row(static_cast<uint32_t>(Imax), static_cast<uint32_t>(V), static_cast<uint32_t>(I[k]));
        h.max_ratio = std::max(h.max_ratio, h.rows[k].ratio);
        h.Bmax = std::max(h.Bmax, B);
        rows[k] = MixedRow{w, static_cast<uint32_t>(__builtin_ctzll(B)), static_cast<uint32_t>(I[k]), static_cast<uint32_t>(R[k]),
                           static_cast<uint32_t>(g_off[k]), static_cast<uint32_t>(hist_off[k])};
    }
    if (std::all_of(rows.begin(), rows.end(), [&](const MixedRow& r) { return r.I == rows[0].I && r.R == rows[0].R; })) h.alike = rows[0];
    GR4PM_TRY(h.d_G.alloc(G.size()));
    GR4PM_TRY(h.d_rows.alloc(K));
    GR4PM_TRY(h.d_w.alloc(K));
    GR4PM_TRY(h.d_G.upload(G.data(), G.size(), h.stream));
    GR4PM_TRY(h.d_rows.upload(rows.data(), K, h.stream));
    GR4PM_TRY(h.d_w.upload(h.words.data(), K, h.stream));
    for (auto& d : h.d_hist) {
        GR4PM_TRY(d.alloc(hist_items));
        GR4PM_TRY(d.zero(h.stream));
    }
    if (assemble_lds(h.Bmax) > 48 * 1024) // Bmax = 512
        GR4PM_TRY(raise_dynamic_lds({reinterpret_cast<const void*>(&k_fft_duc_mixed_assemble), reinterpret_cast<const void*>(&k_fft_duc_assemble)},
                                    assemble_lds(h.Bmax), name));
    GR4PM_HIP_TRY(hipStreamSynchronize(h.stream)); // the uploads read this function's vectors
    return GR4PM_OK;
}

gr4pm_status check_slots(const FftDucBank& h, size_t slots)
{
    if (!fft_duc_mixed_slots_fit(slots, h.max_ratio)) {
        set_error("%s: %zu slots of %u items in the longest row in one call, at most 2^40 items", h.name, slots, h.max_ratio);
        return GR4PM_ERR_OVERFLOW;
    }
    return GR4PM_OK;
}

// a process_iq()'s format: one of the three integer ones (iq::kC64 is the bank's name for complex64, not the ABI's)
gr4pm_status check_format(const FftDucBank& h, int format)
{
    if (!iq::valid(format)) {
        set_error("%s: format %d is none of GR4PM_IQ_SC16 / SC8 / CU8", h.name, format);
        return GR4PM_ERR_INVALID;
    }
    return GR4PM_OK;
}

// the same bound in the FftDuc's words, where a slot is an item: its fronts ask this before the bank asks check_slots()
gr4pm_status check_items(size_t n_in)
{
    if (n_in > (size_t(1) << 40)) {
        set_error("fft_duc: %zu items per row in one call, at most 2^40", n_in);
        return GR4PM_ERR_OVERFLOW;
    }
    return GR4PM_OK;
}

gr4pm_status output_items(const FftDucBank& h, size_t slots, size_t* n_out)
{
    *n_out = 0;
    GR4PM_TRY(check_slots(h, slots));
    *n_out = fft_duc_plan(h.shape, h.taken, slots).samples;
    return GR4PM_OK;
}

// The call of both handles, process() and process_iq(): `slots` slots of every row, row k's items at in + k in_stride;
// format iq::kC64 for complex64 samples, else out and out_cap count items of the format
gr4pm_status process(FftDucBank& h, const gr4pm_c64* in, size_t in_stride, size_t slots, void* out, int format, float gain, size_t out_cap,
                     size_t* n_out, unsigned long long* clipped)
{
    *n_out = 0;
    if (format != iq::kC64 && gain == 0.0f) gain = iq::default_gain(format);
    GR4PM_TRY(check_slots(h, slots));
    if (slots == 0) return GR4PM_OK;
    const FftDucPlan p = fft_duc_plan(h.shape, h.taken, slots); // in slots: a row's items are its ratio times these
    if (p.samples > out_cap) {
        set_error("%s: %zu samples, room for %zu", h.name, p.samples, out_cap);
        return GR4PM_ERR_OVERFLOW;
    }
    const size_t longest = slots * h.max_ratio;
    if (!in || (p.samples && !out) || (h.K > 1 && in_stride < longest)) {
        set_error("%s: no input or output array, or a row stride of %zu items for %zu items", h.name, in_stride, longest);
        return GR4PM_ERR_INVALID;
    }
    const float2* hist = h.d_hist[h.cur].p;
    float2* hist_new = h.d_hist[1 - h.cur].p;
    const uint32_t Imax = static_cast<uint32_t>(h.Imax);
    MixedAsmArgs a = {};
    a.hist = hist, a.in = reinterpret_cast<const float2*>(in), a.in_stride = in_stride;
    a.G = h.d_G.p, a.tw = h.d_tw.p, a.rows = h.d_rows.p, a.spec = reinterpret_cast<float2*>(h.d_spec.p);
    a.K = static_cast<uint32_t>(h.K), a.Bmax = static_cast<uint32_t>(h.Bmax);
    a.carried = static_cast<uint32_t>(p.carried) * Imax, a.hop = h.shape.hop;
    AsmArgs u = {}; // all rows alike: a slot is an item
    u.hist = hist, u.in = a.in, u.in_stride = in_stride, u.H = p.carried;
    u.G = a.G, u.tw = a.tw, u.w = h.d_w.p, u.spec = a.spec;
    u.K = a.K, u.I = h.alike.I, u.logB = h.alike.logB, u.R = h.alike.R;
    u.hop = h.shape.hop, u.hop_items = h.shape.hop_items;
    InvArgs b = {};
    b.spec = h.d_spec.p, b.tT = h.d_tT.p, b.cc = h.d_cc.p, b.out = reinterpret_cast<cf*>(out);
    b.hop = h.shape.hop, b.V = static_cast<uint32_t>(h.V);
    const size_t lds = assemble_lds(h.Bmax);
    for (size_t done = 0; done < p.n_segments;) {
        const size_t segs = std::min(p.n_segments - done, kChunk);
        a.seg0 = u.seg0 = done;
        a.index0 = u.index0 = static_cast<uint32_t>(fft_duc_item_index(h.shape, h.start_index, p.segments_before + done));
        if (h.alike.logB)
            hipLaunchKernelGGL(k_fft_duc_assemble, dim3(static_cast<unsigned>(segs)), dim3(kAsmThreads), lds, h.stream, u);
        else
            hipLaunchKernelGGL(k_fft_duc_mixed_assemble, dim3(static_cast<unsigned>(segs)), dim3(kAsmThreads), lds, h.stream, a);
        launch_inverse(h, b, done, segs, format, gain, clipped);
        done += segs;
    }
    // the rows' new carried items into the other buffer, p.left slots' worth each (nothing left: no launch, no swap)
    const uint32_t carried_new = static_cast<uint32_t>(p.left) * Imax;
    if (carried_new) {
        const size_t most = static_cast<size_t>(carried_new) * h.max_ratio / Imax; // the longest row's
        hipLaunchKernelGGL(k_fft_duc_mixed_history, dim3(static_cast<unsigned>((most + 255) / 256), static_cast<unsigned>(h.K)), dim3(256),
                           0, h.stream, hist, a.in, in_stride, h.d_rows.p, a.carried, slots * h.Imax, carried_new, hist_new);
    }
    GR4PM_HIP_TRY(hipGetLastError());
    if (carried_new) h.cur = 1 - h.cur;
    h.taken += slots;
    *n_out = p.samples;
    return GR4PM_OK;
}

void destroy(FftDucBank* h)
{
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    delete h;
}

gr4pm_status reset(FftDucBank* h)
{
    if (!h) return GR4PM_ERR_INVALID;
    GR4PM_TRY(h->d_hist[h->cur].zero(h->stream));
    h->taken = 0;
    return GR4PM_OK;
}

gr4pm_status frequencies(const FftDucBank* h, double* out)
{
    if (!h || !out) return GR4PM_ERR_INVALID;
    for (size_t k = 0; k < h->K; ++k) out[k] = folded_frequency(h->words[k]);
    return GR4PM_OK;
}

gr4pm_status sizes(const FftDucBank* h, size_t* overlap, size_t* hop)
{
    if (!h || !overlap || !hop) return GR4PM_ERR_INVALID;
    *overlap = h->V;
    *hop = h->shape.hop;
    return GR4PM_OK;
}

// slots since the last completed segment
gr4pm_status pending(const FftDucBank* h, size_t* slots)
{
    if (!h || !slots) return GR4PM_ERR_INVALID;
    *slots = static_cast<size_t>(h->taken % h->shape.hop_items);
    return GR4PM_OK;
}

} // namespace

// distinct types for the ABI, one bank behind both
struct gr4pm_fft_duc : FftDucBank {};
struct gr4pm_fft_duc_mixed : FftDucBank {};

extern "C" {

gr4pm_status gr4pm_fft_duc_taps(size_t interpolation, size_t taps_per_phase, float* out)
try {
    if (!out) return GR4PM_ERR_INVALID;
    GR4PM_TRY(check_interpolation(interpolation));
    return gr4pm_duc_taps(interpolation, taps_per_phase, 0.25, 0.75, out);
}
GR4PM_ABI_CATCH

// the bank of K equal rows, behind the checks that name this entry's own scalars
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
    if (!p->taps && (p->taps_per_phase < 1 || p->taps_per_phase * I > kN)) {
        set_error("fft_duc: %zu taps per phase at an interpolation of %zu: the prototype has 1 .. %zu taps", p->taps_per_phase, I, kN);
        return GR4PM_ERR_INVALID;
    }
    const size_t L = p->taps ? p->n_taps : p->taps_per_phase * I;
    for (size_t t = 0; p->taps && t < L; ++t)
        if (!std::isfinite(p->taps[t])) {
            set_error("fft_duc: taps[%zu] is not finite", t);
            return GR4PM_ERR_INVALID;
        }
    if (p->overlap >= 0) { // the default is a multiple of 256 that reaches; at most it is too high, which the bank says
        const size_t V = static_cast<size_t>(p->overlap);
        if (V % I) {
            set_error("fft_duc: the overlap %zu is no multiple of the interpolation %zu", V, I);
            return GR4PM_ERR_INVALID;
        }
        if (V <= kN - kFftDucMinHop && V + 1 < L) {
            set_error("fft_duc: the overlap %zu is below the %zu taps' reach of %zu samples", V, L, L - 1);
            return GR4PM_ERR_INVALID;
        }
    }
    std::unique_ptr<gr4pm_fft_duc> h(new (std::nothrow) gr4pm_fft_duc);
    if (!h) return GR4PM_ERR_NOMEM;
    const std::vector<float> taps = p->taps ? std::vector<float>(p->taps, p->taps + L) : std::vector<float>();
    GR4PM_TRY(create_bank(*h, "fft_duc", std::move(words), p->gains, std::vector<size_t>(K, I), std::vector<size_t>(K, R),
                          std::vector<std::vector<float>>(K, taps), p->taps_per_phase, p->overlap, p->start_index, p->stream));
    *out = h.release();
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

void gr4pm_fft_duc_destroy(gr4pm_fft_duc* h)
try {
    destroy(h);
}
GR4PM_ABI_CATCH_VOID

gr4pm_status gr4pm_fft_duc_reset(gr4pm_fft_duc* h)
try {
    return reset(h);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_duc_output_items(const gr4pm_fft_duc* h, size_t n_in, size_t* n_out)
try {
    if (!h || !n_out) return GR4PM_ERR_INVALID;
    *n_out = 0;
    GR4PM_TRY(check_items(n_in));
    return output_items(*h, n_in, n_out);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_duc_frequencies(const gr4pm_fft_duc* h, double* out)
try {
    return frequencies(h, out);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_duc_sizes(const gr4pm_fft_duc* h, size_t* overlap, size_t* hop)
try {
    return sizes(h, overlap, hop);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_duc_pending(const gr4pm_fft_duc* h, size_t* items)
try {
    return pending(h, items);
}
GR4PM_ABI_CATCH

// n_in items per row: n_in slots of one item
gr4pm_status gr4pm_fft_duc_process(gr4pm_fft_duc* h, const gr4pm_c64* in, size_t in_stride, size_t n_in, gr4pm_c64* out,
                                   size_t out_cap, size_t* n_out)
try {
    if (!h || !n_out) return GR4PM_ERR_INVALID;
    *n_out = 0;
    GR4PM_TRY(check_items(n_in));
    return process(*h, in, in_stride, n_in, out, iq::kC64, 0.0f, out_cap, n_out, nullptr);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_duc_process_iq(gr4pm_fft_duc* h, const gr4pm_c64* in, size_t in_stride, size_t n_in, void* out, int format,
                                      float gain, size_t out_cap, size_t* n_out, unsigned long long* clipped)
try {
    if (!h || !n_out) return GR4PM_ERR_INVALID;
    *n_out = 0;
    GR4PM_TRY(check_format(*h, format));
    GR4PM_TRY(check_items(n_in));
    return process(*h, in, in_stride, n_in, out, format, gain, out_cap, n_out, clipped);
}
GR4PM_ABI_CATCH

// ---- MixedFftDuc: an interpolation per row ------------------------------------------------------

gr4pm_status gr4pm_fft_duc_mixed_create(const gr4pm_fft_duc_mixed_params* p, gr4pm_fft_duc_mixed** out)
try {
    if (!p || !out) return GR4PM_ERR_INVALID;
    *out = nullptr;
    const size_t K = p->n_channels;
    std::vector<uint32_t> words;
    GR4PM_TRY(frequency_words("fft_duc_mixed", p->frequencies, K, kFftDucMaxK, words));
    if (!p->interpolations) {
        set_error("fft_duc_mixed: no interpolations");
        return GR4PM_ERR_INVALID;
    }
    if ((p->taps == nullptr) != (p->n_taps == nullptr)) {
        set_error("fft_duc_mixed: taps and n_taps come together or not at all");
        return GR4PM_ERR_INVALID;
    }
    GR4PM_TRY(finite_gains("fft_duc_mixed", p->gains, K));
    std::vector<std::vector<float>> taps(K);
    for (size_t k = 0, at = 0; p->taps && k < K; at += p->n_taps[k], ++k) {
        GR4PM_TRY(prototype_length("fft_duc_mixed", p->taps, p->n_taps[k], kN));
        taps[k].assign(p->taps + at, p->taps + at + p->n_taps[k]);
    }
    std::unique_ptr<gr4pm_fft_duc_mixed> h(new (std::nothrow) gr4pm_fft_duc_mixed);
    if (!h) return GR4PM_ERR_NOMEM;
    GR4PM_TRY(create_bank(*h, "fft_duc_mixed", std::move(words), p->gains, std::vector<size_t>(p->interpolations, p->interpolations + K),
                          p->images ? std::vector<size_t>(p->images, p->images + K) : std::vector<size_t>(K, 2), std::move(taps),
                          p->taps_per_phase, p->overlap, p->start_index, p->stream));
    *out = h.release();
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

void gr4pm_fft_duc_mixed_destroy(gr4pm_fft_duc_mixed* h)
try {
    destroy(h);
}
GR4PM_ABI_CATCH_VOID

gr4pm_status gr4pm_fft_duc_mixed_reset(gr4pm_fft_duc_mixed* h)
try {
    return reset(h);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_duc_mixed_items_for(const gr4pm_fft_duc_mixed* h, size_t slots, size_t* items)
try {
    if (!h || !items) return GR4PM_ERR_INVALID;
    for (size_t k = 0; k < h->K; ++k) items[k] = 0;
    GR4PM_TRY(check_slots(*h, slots));
    for (size_t k = 0; k < h->K; ++k) items[k] = fft_duc_mixed_items(h->rows[k], slots);
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_duc_mixed_output_items(const gr4pm_fft_duc_mixed* h, size_t slots, size_t* n_out)
try {
    if (!h || !n_out) return GR4PM_ERR_INVALID;
    return output_items(*h, slots, n_out);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_duc_mixed_frequencies(const gr4pm_fft_duc_mixed* h, double* out)
try {
    return frequencies(h, out);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_duc_mixed_sizes(const gr4pm_fft_duc_mixed* h, size_t* overlap, size_t* hop)
try {
    return sizes(h, overlap, hop);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_duc_mixed_pending(const gr4pm_fft_duc_mixed* h, size_t* slots)
try {
    return pending(h, slots);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_duc_mixed_process(gr4pm_fft_duc_mixed* h, const gr4pm_c64* in, size_t in_stride, size_t slots, gr4pm_c64* out,
                                         size_t out_cap, size_t* n_out)
try {
    if (!h || !n_out) return GR4PM_ERR_INVALID;
    return process(*h, in, in_stride, slots, out, iq::kC64, 0.0f, out_cap, n_out, nullptr);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_fft_duc_mixed_process_iq(gr4pm_fft_duc_mixed* h, const gr4pm_c64* in, size_t in_stride, size_t slots, void* out,
                                            int format, float gain, size_t out_cap, size_t* n_out, unsigned long long* clipped)
try {
    if (!h || !n_out) return GR4PM_ERR_INVALID;
    *n_out = 0;
    GR4PM_TRY(check_format(*h, format));
    return process(*h, in, in_stride, slots, out, format, gain, out_cap, n_out, clipped);
}
GR4PM_ABI_CATCH

} // extern "C"
