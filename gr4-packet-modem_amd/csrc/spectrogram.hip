// spectrogram.hip -- PSD rows over time of one wideband stream, the power of bands of those rows, and the host-only burst
// finder made from it.  The project's own block (the reference has none).  Definition (include/gr4pm_hip.h, DESIGN.md
// section 21): the Spectrum's segments (spectrum.hip), and with R = average
//     row t = the segments t R .. t R + R - 1;  mean: fl32(sum_s |X_s[k]|^2 . inv),  max: fl32(max_s |X_s[k]|^2 . inv)
//
// k_spectrogram_w64<format, detector>: one wave walks a run of consecutive units (hostlogic/spectrogram_plan.hpp: a unit
//   is a row, or the part of a row that lies in this call) segment by segment, back to back across the rows, and does
//   per segment what k_spectrum_w64 does: load in rows of 64 samples, window from LDS, dft32, w64_store,
//   w64_mid_dev<1, true>, dft32, powers in the registers where the outputs land.  It keeps 32 accumulators, a sum OR a
//   maximum: the detector is a template parameter.  With 32 registers fewer than k_spectrum_w64's sums and maxima, both
//   halves of the next segment are requested when the exchange has freed pass A's registers and arrive while pass B
//   runs (234 registers for the sum, 222 for the maximum, no scratch; the Spectrum's one half then, one half after pass
//   B has 220 here and measures the same within the spread).  The first segment of a
//   row initialises them (sum = p, max = p: no 0 + p and no max(0, p), so R = 1 gives the same bits for both detectors);
//   only the call's unit 0 may start from the carried accumulators instead.  After R segments the wave multiplies by inv
//   and stores the row coalesced (lane + 64 j); the wave whose run ends inside a row writes the raw accumulators to the
//   new carry.  Carry in and carry out are two buffers (read old, write new), as the stream tail's are: the wave of
//   unit 0 and the wave of the last unit are different waves in general.
//   The LDS image is k_spectrum_w64's (twiddles | eight exchange buffers | the window), two waves per SIMD.
// k_band_power: one wave per row reads it once (lane + 64 j), every lane adds its in-band bins in double in ascending j,
//   and a butterfly over the wave follows, the same order in every call: no atomic, the same call gives the same bits.
// The carried samples are stream_tail.hpp's, exactly as in spectrum.hip.  Built with FFT_FLAGS like spectrum.o: a
// segment's powers are the Spectrum's expressions.
#include "spectrum_segment.hpp"
#include "hostlogic/burst_find.hpp"
#include "hostlogic/spectrogram_plan.hpp"

#include <algorithm>
#include <cmath>

namespace {

namespace iq = gr4pm::iq;
using namespace gr4pm;
using gr4pm::hostlogic::spectrogram_plan;
using gr4pm::hostlogic::SpectrogramPlan;

constexpr size_t kN = kFftN;
constexpr size_t kMaxBands = 64;
constexpr int kBandWaves = 4; // rows per workgroup of k_band_power

struct SgramArgs {
    const float2* hist; // the H carried samples in front of in[0]
    const void* in;     // complex64, or items of the kernel's integer format
    size_t H;
    const float* window;
    const float4* tT;
    const cf* cc;
    const float* carry_old; // [2048] raw accumulators of the incomplete row before the call
    float* carry_new;       // [2048] ... after it
    float* rows;            // [n_rows][2048]
    size_t n_seg;           // segments of the call
    size_t units;           // rows, plus the incomplete one
    size_t run;             // units per wave
    uint32_t carry_in;      // segments in the carried row, < R
    uint32_t reads_carry;   // unit 0 starts from carry_old
    uint32_t R;
    uint32_t hop;
    float scale;            // of an integer format's unpack
    float inv;              // 1 / (R sum w^2), or 1 / sum w^2 for the maximum
};

template <int F, int DET>
__global__ __launch_bounds__(kW64Threads, 2) void k_spectrogram_w64(SgramArgs a)
{
    __shared__ float4 lds4[kW64LdsF4 + kFftN / 4]; // twiddles | eight exchange buffers | the window
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < kW64TwFloat4; i += kW64Threads) lds4[i] = a.tT[i];
    for (int i = tid; i < kFftN / 4; i += kW64Threads) lds4[kW64LdsF4 + i] = reinterpret_cast<const float4*>(a.window)[i];
    __syncthreads(); // the only workgroup-wide synchronisation of the kernel
    float4* xb4 = lds4 + kW64TwFloat4 + wave * kW64BufF4;
    const uint32_t base = __builtin_amdgcn_readfirstlane(
        static_cast<uint32_t>(reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) char*)xb4)));
    const float4* row = xb4 + (lane & 31) * (kW64Row / 4);
    const float4* ldsT = lds4;
    const cf c = a.cc[lane];

    const uint32_t w = blockIdx.x * kW64Waves + wave;
    size_t u = static_cast<size_t>(w) * a.run; // the unit the wave is in
    if (u >= a.units) return;
    const size_t u_end = a.units - u < a.run ? a.units : u + a.run;
    // units u .. u_end - 1 are the call's segments [first, end)
    const size_t first = u == 0 ? 0 : u * a.R - a.carry_in;
    const size_t end = u_end * a.R - a.carry_in < a.n_seg ? u_end * a.R - a.carry_in : a.n_seg;

    const float* wl = reinterpret_cast<const float*>(lds4 + kW64LdsF4) + lane; // w[lane + 64 j]: a row of 64 per read
    float acc[32];
    uint32_t k = 0; // segments in acc
    if (u == 0 && a.reads_carry) {
        k = a.carry_in;
#pragma unroll
        for (int j = 0; j < 32; ++j) acc[j] = a.carry_old[lane + 64 * j];
    } else {
#pragma unroll
        for (int j = 0; j < 32; ++j) acc[j] = 0.0f; // overwritten by the row's first segment
    }
    // segment `seg` of the call begins at the virtual item seg hop
    auto load_half = [&](cf* dst, size_t seg, int h) { load_half_segment<F>(dst, a.hist, a.H, a.in, a.scale, seg * a.hop, lane, h); };

    cf X[32];
    load_half(X, first, 0);
    load_half(X, first, 1);
    for (size_t s = first; s < end; ++s) {
#pragma unroll
        for (int j = 0; j < 32; ++j) X[j] = X[j] * dup_x(mk(wl[64 * j], 0.0f));
        cf bq[32];
        dft32(X);
        w64_store(X, base);
        w64_mid_dev<1, true>(lane, row, ldsT, c, bq);
        // pass A's registers are dead: they take the whole next segment, which arrives while pass B runs
        const bool has_next = s + 1 < end;
        if (has_next) {
            load_half(X, s + 1, 0);
            load_half(X, s + 1, 1);
        }
        dft32(bq);
        const bool opens = k == 0; // uniform: the row's first segment
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const float p = fmaf(bq[j].y, bq[j].y, bq[j].x * bq[j].x);
            if constexpr (DET == GR4PM_SPECTROGRAM_MEAN)
                acc[j] = opens ? p : acc[j] + p;
            else
                acc[j] = opens ? p : __builtin_fmaxf(acc[j], p);
        }
        if (++k == a.R) { // the row is complete: one product, then rows of 64 floats
            float* out = a.rows + u * kFftN + lane;
#pragma unroll
            for (int j = 0; j < 32; ++j) out[64 * j] = acc[j] * a.inv;
            ++u;
            k = 0;
        }
    }
    if (k) { // the call ends inside this row (only the last unit can: spectrogram_plan's writes_carry)
        float* out = a.carry_new + lane;
#pragma unroll
        for (int j = 0; j < 32; ++j) out[64 * j] = acc[j];
    }
}

struct BandArgs {
    const float* rows; // [n_rows][2048]
    double* out;       // [n_bands][n_rows]
    size_t n_rows;
    uint32_t n_bands;
    uint32_t first[kMaxBands]; // < 2048
    uint32_t count[kMaxBands]; // 1 .. 2048
};

// one wave per row; lane l holds the bins l + 64 j
__global__ __launch_bounds__(kBandWaves * 64) void k_band_power(BandArgs a)
{
    const int lane = threadIdx.x & 63;
    const size_t r = static_cast<size_t>(blockIdx.x) * kBandWaves + (threadIdx.x >> 6);
    if (r >= a.n_rows) return;
    const float* p = a.rows + r * kFftN + lane;
    float v[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) v[j] = p[64 * j];
    for (uint32_t b = 0; b < a.n_bands; ++b) {
        const uint32_t first = a.first[b], count = a.count[b];
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 32; ++j) { // bin k is in the band iff (k - first) mod 2048 < count
            const uint32_t d = (static_cast<uint32_t>(lane + 64 * j) - first) & (kFftN - 1);
            s += d < count ? static_cast<double>(v[j]) : 0.0;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64); // a + b = b + a: every lane holds the same sum
        if (lane == 0) a.out[static_cast<size_t>(b) * a.n_rows + r] = s;
    }
}

} // namespace

struct gr4pm_spectrogram {
    size_t hop = 0, average = 1;
    int detector = GR4PM_SPECTROGRAM_MEAN;
    uint64_t taken = 0;    // T: samples since create or reset
    uint64_t segments = 0;
    float inv = 0.0f;      // fl32(1 / (R sum w^2)), for the maximum fl32(1 / sum w^2)
    hipStream_t stream = nullptr;
    gr4pm::SegmentTransform tf; // the window and its power, the transform's tables, the waves of one launch
    gr4pm::StreamTail tail;     // keep = 0, frame = N: the samples of the incomplete segment
    int carry_cur = 0;          // which buffer holds the incomplete row
    gr4pm::DevBuf<float> d_carry[2];
};

template <int F>
static void launch_rows(int detector, unsigned blocks, hipStream_t stream, const SgramArgs& a)
{
    if (detector == GR4PM_SPECTROGRAM_MEAN)
        hipLaunchKernelGGL((k_spectrogram_w64<F, GR4PM_SPECTROGRAM_MEAN>), dim3(blocks), dim3(kW64Threads), 0, stream, a);
    else
        hipLaunchKernelGGL((k_spectrogram_w64<F, GR4PM_SPECTROGRAM_MAX>), dim3(blocks), dim3(kW64Threads), 0, stream, a);
}

// process() and process_iq(): format iq::kC64 for complex64 samples
static gr4pm_status process_any(gr4pm_spectrogram* h, const void* x, int format, float scale, size_t n, float* rows,
                                size_t rows_cap, size_t* n_rows)
{
    if (n_rows) *n_rows = 0;
    if (!h) return GR4PM_ERR_INVALID;
    if (n > (size_t(1) << 40)) {
        set_error("spectrogram: %zu samples in one call, at most 2^40", n);
        return GR4PM_ERR_OVERFLOW;
    }
    if (n == 0) return GR4PM_OK;
    if (!x) {
        set_error("spectrogram: no input array");
        return GR4PM_ERR_INVALID;
    }
    const SpectrogramPlan p = spectrogram_plan(h->taken, n, kN, h->hop, h->average, h->tf.max_waves);
    if (p.rows > rows_cap) {
        set_error("spectrogram: the call completes %zu rows, room for %zu", p.rows, rows_cap);
        return GR4PM_ERR_OVERFLOW;
    }
    if (p.rows && !rows) {
        set_error("spectrogram: no array for the rows");
        return GR4PM_ERR_INVALID;
    }
    const StreamTail::Plan t = {h->tail.d_hist[h->tail.cur].p, h->tail.d_hist[1 - h->tail.cur].p, p.seg.tail, p.seg.n_segments,
                                p.seg.tail_new, p.seg.tail_new};
    SgramArgs a = {};
    a.hist = t.hist, a.in = x, a.H = p.seg.tail;
    a.window = h->tf.d_window.p, a.tT = h->tf.d_tT.p, a.cc = h->tf.d_cc.p;
    a.carry_old = h->d_carry[h->carry_cur].p, a.carry_new = h->d_carry[1 - h->carry_cur].p, a.rows = rows;
    a.n_seg = p.seg.n_segments, a.units = p.units, a.run = p.run;
    a.carry_in = static_cast<uint32_t>(p.carry_in), a.reads_carry = p.reads_carry ? 1u : 0u;
    a.R = static_cast<uint32_t>(h->average), a.hop = static_cast<uint32_t>(h->hop), a.scale = scale, a.inv = h->inv;
    iq::with_format(format, [&](auto f) {
        if (p.units)
            launch_rows<decltype(f)::value>(h->detector, static_cast<unsigned>((p.waves + kW64Waves - 1) / kW64Waves), h->stream, a);
        h->tail.launch_history<decltype(f)::value>(t, x, 0, n, scale, h->stream);
    });
    GR4PM_HIP_TRY(hipGetLastError());
    h->tail.commit(t);
    if (p.writes_carry) h->carry_cur = 1 - h->carry_cur;
    h->taken += n;
    h->segments += p.seg.n_segments;
    if (n_rows) *n_rows = p.rows;
    return GR4PM_OK;
}

extern "C" {

gr4pm_status gr4pm_spectrogram_create(const gr4pm_spectrogram_params* p, gr4pm_spectrogram** out)
try {
    if (!p || !out) return GR4PM_ERR_INVALID;
    *out = nullptr;
    if (p->fft_size != kN) {
        set_error("spectrogram: fft_size %u, only 2048 exists", p->fft_size);
        return GR4PM_ERR_INVALID;
    }
    if (p->hop == 0 || p->hop > kN) {
        set_error("spectrogram: hop %u, need 1 .. %zu", p->hop, kN);
        return GR4PM_ERR_INVALID;
    }
    if (p->average == 0 || p->average > gr4pm_spectrum_float_run()) {
        set_error("spectrogram: average %u, need 1 .. %u", p->average, gr4pm_spectrum_float_run());
        return GR4PM_ERR_INVALID;
    }
    if (p->detector != GR4PM_SPECTROGRAM_MEAN && p->detector != GR4PM_SPECTROGRAM_MAX) {
        set_error("spectrogram: detector %u is neither GR4PM_SPECTROGRAM_MEAN nor GR4PM_SPECTROGRAM_MAX", p->detector);
        return GR4PM_ERR_INVALID;
    }
    std::unique_ptr<gr4pm_spectrogram> h(new (std::nothrow) gr4pm_spectrogram);
    if (!h) return GR4PM_ERR_NOMEM;
    h->hop = p->hop;
    h->average = p->average;
    h->detector = static_cast<int>(p->detector);
    h->stream = static_cast<hipStream_t>(p->stream);
    GR4PM_TRY(h->tf.create(p->window, h->stream, "spectrogram"));
    h->inv = static_cast<float>(1.0 / ((h->detector == GR4PM_SPECTROGRAM_MEAN ? static_cast<double>(p->average) : 1.0) * h->tf.window_power));
    for (auto& d : h->d_carry) {
        GR4PM_TRY(d.alloc(kN));
        GR4PM_TRY(d.zero(h->stream));
    }
    GR4PM_TRY(h->tail.alloc(0, kN, 1, h->stream));
    return finish_create(h, out, "spectrogram");
}
GR4PM_ABI_CATCH

void gr4pm_spectrogram_destroy(gr4pm_spectrogram* h)
try {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    delete h;
}
GR4PM_ABI_CATCH_VOID

gr4pm_status gr4pm_spectrogram_reset(gr4pm_spectrogram* h)
try {
    if (!h) return GR4PM_ERR_INVALID;
    GR4PM_TRY(h->tail.reset(h->stream));
    h->taken = 0; // no segment counted: the next row starts from its first segment, not from a carry
    h->segments = 0;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_spectrogram_rows(const gr4pm_spectrogram* h, size_t n, size_t* rows)
try {
    if (!h || !rows) return GR4PM_ERR_INVALID;
    *rows = spectrogram_plan(h->taken, n, kN, h->hop, h->average, h->tf.max_waves).rows;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_spectrogram_process(gr4pm_spectrogram* h, const void* x, size_t n, float* rows, size_t rows_cap, size_t* n_rows)
try {
    return process_any(h, x, iq::kC64, 0.0f, n, rows, rows_cap, n_rows);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_spectrogram_process_iq(gr4pm_spectrogram* h, const void* x, int format, float scale, size_t n, float* rows,
                                          size_t rows_cap, size_t* n_rows)
try {
    if (!iq::valid(format)) {
        set_error("spectrogram: format %d is none of GR4PM_IQ_SC16 / SC8 / CU8", format);
        return GR4PM_ERR_INVALID;
    }
    return process_any(h, x, format, scale == 0.0f ? iq::default_scale(format) : scale, n, rows, rows_cap, n_rows);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_spectrogram_band_power(gr4pm_spectrogram* h, const float* rows, size_t n_rows, const gr4pm_band* bands,
                                          size_t n_bands, double* out)
try {
    if (!h) return GR4PM_ERR_INVALID;
    if (n_bands > kMaxBands) {
        set_error("spectrogram: %zu bands in one call, at most %zu", n_bands, kMaxBands);
        return GR4PM_ERR_INVALID;
    }
    if (n_bands && !bands) return GR4PM_ERR_INVALID;
    BandArgs a = {};
    for (size_t b = 0; b < n_bands; ++b) {
        if (bands[b].first_bin >= kN || bands[b].n_bins == 0 || bands[b].n_bins > kN) {
            set_error("spectrogram: band %zu is %u bins from bin %u, need 1 .. %zu bins from a bin below %zu", b, bands[b].n_bins,
                      bands[b].first_bin, kN, kN);
            return GR4PM_ERR_INVALID;
        }
        a.first[b] = bands[b].first_bin, a.count[b] = bands[b].n_bins;
    }
    if (n_rows > (size_t(1) << 32)) {
        set_error("spectrogram: %zu rows in one call, at most 2^32", n_rows);
        return GR4PM_ERR_OVERFLOW;
    }
    if (!n_rows || !n_bands) return GR4PM_OK;
    if (!rows || !out) {
        set_error("spectrogram: band_power needs the rows and an output array");
        return GR4PM_ERR_INVALID;
    }
    a.rows = rows, a.out = out, a.n_rows = n_rows, a.n_bands = static_cast<uint32_t>(n_bands);
    hipLaunchKernelGGL(k_band_power, dim3(static_cast<unsigned>((n_rows + kBandWaves - 1) / kBandWaves)), dim3(kBandWaves * 64), 0,
                       h->stream, a);
    GR4PM_HIP_TRY(hipGetLastError());
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_find_bursts(const double* power, size_t n, const gr4pm_burst_params* p, gr4pm_burst* out, size_t cap,
                               size_t* count)
try {
    if (count) *count = 0;
    if (!power || !n || !p || !count || (cap && !out)) return GR4PM_ERR_INVALID;
    if (!(p->threshold_db > 0.0)) {
        set_error("find_bursts: threshold_db must be positive");
        return GR4PM_ERR_INVALID;
    }
    if (!std::isfinite(p->floor) || p->floor < 0.0) {
        set_error("find_bursts: floor must be finite and not negative (0: the lower median)");
        return GR4PM_ERR_INVALID;
    }
    *count = hostlogic::find_bursts(power, n, p->threshold_db, p->floor, p->max_gap_rows, p->min_rows, out, cap);
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

} // extern "C"
