// line_spectrum.hip -- the Welch spectrum of a memoryless nonlinearity of rows of channel items, whose line gives a
// burst's residual carrier offset (x^4, x^2) or its symbol rate (|x|^2); the host-only line finder and the rational
// approximation that go with it.  The project's own block (the reference has none).  Definition: include/gr4pm_hip.h,
// DESIGN.md section 23; the row, segment and run arithmetic: hostlogic/line_plan.hpp, whose expressions the kernels use.
//
// k_line_spectrum_w64<statistic>: the Spectrum's workgroup (spectrum.hip: eight waves on the one-exchange transform of
//   fft2048_w64.hpp, the window in LDS, register j of lane l holds index l + 64 j on both sides of the transform), but a
//   wave takes a run of at most 64 consecutive transforms of ONE row, found from the call's run starts, which travel by
//   value beside the rows' lengths.  The nonlinearity is applied in the registers where a segment's samples land, with the
//   window product.  A segment that lies wholly below the row's length is loaded unguarded under a wave-uniform branch; of
//   any other, an item at or beyond the length is not loaded at all (load_row_half: the row may end at the buffer's end).
//   Only 32 sums live across a run (no maxima).  The first segment of an envelope pair is prefetched as the Spectrum's
//   next segment is (half when the exchange has freed pass A's registers, half when pass B is complete); the second is
//   requested where the transform begins, into the registers pass B takes afterwards, and (|a|^2, |b|^2) w is formed
//   there.  Both segments of the pair prefetched during pass B spill 145 registers.
// k_line_spectrum_reduce: per row and bin pair (k, N - k) the runs' partials in run order in float64, on from the handle's
//   acc[64][2048] when an earlier launch of the call began the row; the launch that ends a row folds (envelope), divides
//   by S_r sum w^2 and writes out[r].  No floating-point atomic; a row's bits depend on that row alone.
// Built with FFT_FLAGS, as spectrum.o: the transform and the nonlinearity may contract to FMA.
#include "spectrum_segment.hpp"
#include "hostlogic/line_find.hpp"
#include "hostlogic/line_plan.hpp"
#include "hostlogic/ratio.hpp"

#include <algorithm>
#include <cmath>

namespace {

using namespace gr4pm;
namespace hl = gr4pm::hostlogic;

constexpr size_t kN = kFftN;
static_assert(hl::kLineN == kFftN, "line_plan.hpp is written for the 2048-point transform");

struct LineArgs {
    const cf* x;
    size_t stride;
    const float* gains; // DEVICE, or nullptr for 1
    const float* window;
    const float4* tT;
    const cf* cc;
    float* part;        // [waves of the launch][2048]
    double* acc;        // [64][2048]: rows that go on in a later launch
    double* out;        // [R][2048]
    double window_power;
    uint64_t w0;        // the launch's first wave, counted over the call
    uint32_t n_waves;   // of the launch
    uint32_t R;
    uint32_t hop;
    uint64_t lengths[hl::kLineMaxRows];
    uint64_t run_start[hl::kLineMaxRows + 1];
};

// Half h (0 or 1) of the segment that begins at item i0 of a row whose items below `limit` exist: register j of lane l
// takes item i0 + l + 64 j, j = 16 h .. 16 h + 15, or zero where that item is at or beyond the limit -- which is then not
// loaded.  i0 and limit are wave-uniform.  The row comes by reference, as load_half_segment's stream does.
__device__ __forceinline__ void load_row_half(cf* dst, const cf* const& x, uint64_t i0, uint64_t limit, int lane, int h)
{
    int ln = lane;
    asm volatile("" : "+v"(ln)); // addresses are formed here, not hoisted out of the run's loop
    if (hl::line_unguarded(i0, limit)) { // uniform: the whole segment lies inside the row
        const cf* p = x + i0 + ln;
#pragma unroll
        for (int j = 16 * h; j < 16 * h + 16; ++j) dst[j] = p[64 * j];
    } else {
#pragma unroll
        for (int j = 16 * h; j < 16 * h + 16; ++j) {
            const uint64_t i = static_cast<uint64_t>(ln + 64 * j);
            dst[j] = mk(0.0f, 0.0f);
            if (hl::line_item_loaded(i0, i, limit)) dst[j] = x[i0 + i];
        }
    }
}

// u = g x, one product per component; u^2 = (ux^2 - uy^2, 2 ux uy)
__device__ __forceinline__ cf line_square(float re, float im) { return mk(re * re - im * im, 2.0f * re * im); }

template <int S>
__device__ __forceinline__ cf line_value(cf x, float g)
{
    const float ux = g * x.x, uy = g * x.y;
    if constexpr (S == GR4PM_LINE_SQUARE) {
        return line_square(ux, uy);
    } else {
        const cf v = line_square(ux, uy);
        return line_square(v.x, v.y);
    }
}
__device__ __forceinline__ float line_envelope(cf x, float g)
{
    const float ux = g * x.x, uy = g * x.y;
    return ux * ux + uy * uy;
}

template <int S>
__global__ __launch_bounds__(kW64Threads, 2) void k_line_spectrum_w64(LineArgs a)
{
    constexpr bool kPairs = S == GR4PM_LINE_ENVELOPE;
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

    const uint32_t wl_ = blockIdx.x * kW64Waves + wave; // of the launch
    if (wl_ >= a.n_waves) return;
    const uint64_t w = a.w0 + wl_;
    const uint32_t r = hl::line_row_of(a.run_start, a.R, w);
    const uint64_t n_r = a.lengths[r];
    const uint64_t hop = a.hop;
    const uint64_t segments = hl::line_segments(n_r, hop);
    const uint64_t first = (w - a.run_start[r]) * hl::kLineFloatRun; // the run's first transform
    const uint32_t count = static_cast<uint32_t>(hl::line_run_count(hl::line_transforms(segments, kPairs), w - a.run_start[r]));
    const cf* xr = a.x + static_cast<size_t>(r) * a.stride;
    const float g = a.gains ? a.gains[r] : 1.0f;

    const float* wl = reinterpret_cast<const float*>(lds4 + kW64LdsF4) + lane; // w[lane + 64 j]: a row of 64 per read
    float sum[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) sum[j] = 0.0f;

    // transform t of the row: segment t, or for the envelope the segments 2 t (prefetched into X) and 2 t + 1
    cf X[32];
    auto load_half = [&](uint64_t t, int h) {
        const uint64_t seg = kPairs ? 2 * t : t;
        load_row_half(X, xr, seg * hop, hl::line_segment_limit(seg, segments, n_r), lane, h);
    };
    load_half(first, 0);
    load_half(first, 1);
    for (uint32_t s = 0; s < count; ++s) {
        cf bq[32];
        if constexpr (kPairs) { // the pair's second segment, in the registers pass B takes afterwards
            const uint64_t seg = 2 * (first + s) + 1, limit = hl::line_segment_limit(seg, segments, n_r);
            load_row_half(bq, xr, seg * hop, limit, lane, 0);
            load_row_half(bq, xr, seg * hop, limit, lane, 1);
        }
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            if constexpr (kPairs)
                X[j] = mk(line_envelope(X[j], g), line_envelope(bq[j], g)) * dup_x(mk(wl[64 * j], 0.0f));
            else
                X[j] = line_value<S>(X[j], g) * dup_x(mk(wl[64 * j], 0.0f));
        }
        dft32(X);
        w64_store(X, base);
        w64_mid_dev<1, true>(lane, row, ldsT, c, bq);
        // pass A's registers are dead: they take the next transform's samples -- one half now, which arrives while pass B
        // runs, the other when pass B is complete (the pin: hipcc otherwise hoists those loads above the arithmetic)
        const bool has_next = s + 1 < count;
        if (has_next) load_half(first + s + 1, 0);
        dft32(bq);
#pragma unroll
        for (int k = 0; k < 32; k += 4) w64_pin4(bq + k);
        if (has_next) load_half(first + s + 1, 1);
#pragma unroll
        for (int j = 0; j < 32; ++j) sum[j] += fmaf(bq[j].y, bq[j].y, bq[j].x * bq[j].x);
    }
    float* ps = a.part + static_cast<size_t>(wl_) * kFftN + lane;
#pragma unroll
    for (int j = 0; j < 32; ++j) ps[64 * j] = sum[j];
}

// grid (17, R) of 64 threads: thread k <= 1024 of a row takes the bins k and (N - k) mod N
template <bool kPairs>
__global__ __launch_bounds__(64) void k_line_spectrum_reduce(LineArgs a)
{
    const uint32_t k = blockIdx.x * 64 + threadIdx.x;
    if (k > kFftN / 2) return;
    const uint32_t k2 = (kFftN - k) % kFftN;
    const uint32_t r = blockIdx.y;
    const uint64_t rs = a.run_start[r], re = a.run_start[r + 1], end = a.w0 + a.n_waves;
    double* o = a.out + static_cast<size_t>(r) * kFftN;
    if (rs == re) { // no segment: zeros, written by the call's first launch
        if (a.w0 == 0) o[k] = 0.0, o[k2] = 0.0;
        return;
    }
    const uint64_t lo = rs > a.w0 ? rs : a.w0, hi = re < end ? re : end;
    if (lo >= hi) return; // none of the row's runs is in this launch
    double* ac = a.acc + static_cast<size_t>(r) * kFftN;
    double s = 0.0, t = 0.0;
    if (rs < a.w0) s = ac[k], t = ac[k2];
    const float* p = a.part + static_cast<size_t>(lo - a.w0) * kFftN;
    for (uint64_t w = lo; w < hi; ++w, p += kFftN) { // in run order
        s += static_cast<double>(p[k]);
        t += static_cast<double>(p[k2]);
    }
    if (re > end) { // the row goes on in the next launch
        ac[k] = s, ac[k2] = t;
        return;
    }
    const double den = static_cast<double>(hl::line_segments(a.lengths[r], a.hop)) * a.window_power;
    if constexpr (kPairs) {
        const double v = (s + t) * 0.5 / den;
        o[k] = v, o[k2] = v;
    } else {
        o[k] = s / den, o[k2] = t / den;
    }
}

} // namespace

struct gr4pm_line_spectrum {
    size_t hop = 0;
    hipStream_t stream = nullptr;
    gr4pm::SegmentTransform tf; // the window and its power, the transform's tables, the waves of one launch
    gr4pm::DevBuf<float> d_part;
    gr4pm::DevBuf<double> d_acc;
};

template <int S>
static void launch_all(gr4pm_line_spectrum* h, LineArgs& a, uint64_t total)
{
    uint64_t done = 0;
    do { // once even without any run: the reduce writes the zeros of rows without a segment
        const uint64_t waves = std::min<uint64_t>(h->tf.max_waves, total - done);
        a.w0 = done, a.n_waves = static_cast<uint32_t>(waves);
        if (waves)
            hipLaunchKernelGGL(k_line_spectrum_w64<S>, dim3(static_cast<unsigned>((waves + kW64Waves - 1) / kW64Waves)),
                               dim3(kW64Threads), 0, h->stream, a);
        hipLaunchKernelGGL(k_line_spectrum_reduce<S == GR4PM_LINE_ENVELOPE>, dim3(kFftN / 2 / 64 + 1, a.R), dim3(64), 0,
                           h->stream, a);
        done += waves;
    } while (done < total);
}

extern "C" {

uint32_t gr4pm_line_spectrum_float_run(void)
try {
    return static_cast<uint32_t>(hl::kLineFloatRun);
}
GR4PM_ABI_CATCH_RET(0)

gr4pm_status gr4pm_line_spectrum_create(const gr4pm_line_spectrum_params* p, gr4pm_line_spectrum** out)
try {
    if (!p || !out) return GR4PM_ERR_INVALID;
    *out = nullptr;
    if (p->fft_size != kN) {
        set_error("line_spectrum: fft_size %u, only 2048 exists", p->fft_size);
        return GR4PM_ERR_INVALID;
    }
    if (p->hop == 0 || p->hop > kN) {
        set_error("line_spectrum: hop %u, need 1 .. %zu", p->hop, kN);
        return GR4PM_ERR_INVALID;
    }
    std::unique_ptr<gr4pm_line_spectrum> h(new (std::nothrow) gr4pm_line_spectrum);
    if (!h) return GR4PM_ERR_NOMEM;
    h->hop = p->hop;
    h->stream = static_cast<hipStream_t>(p->stream);
    GR4PM_TRY(h->tf.create(p->window, h->stream, "line_spectrum"));
    GR4PM_TRY(h->d_part.alloc(h->tf.max_waves * kN));
    GR4PM_TRY(h->d_acc.alloc(hl::kLineMaxRows * kN));
    return finish_create(h, out, "line_spectrum");
}
GR4PM_ABI_CATCH

void gr4pm_line_spectrum_destroy(gr4pm_line_spectrum* h)
try {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    delete h;
}
GR4PM_ABI_CATCH_VOID

gr4pm_status gr4pm_line_spectrum_process(gr4pm_line_spectrum* h, const gr4pm_c64* x, size_t stride, size_t n_cols,
                                         const uint64_t* lengths, size_t n_rows, const float* gains, int statistic, double* out)
try {
    if (!h) return GR4PM_ERR_INVALID;
    if (n_rows > hl::kLineMaxRows) {
        set_error("line_spectrum: %zu rows in one call, at most %zu", n_rows, hl::kLineMaxRows);
        return GR4PM_ERR_INVALID;
    }
    if (statistic != GR4PM_LINE_ENVELOPE && statistic != GR4PM_LINE_SQUARE && statistic != GR4PM_LINE_FOURTH) {
        set_error("line_spectrum: statistic %d is none of GR4PM_LINE_ENVELOPE / SQUARE / FOURTH", statistic);
        return GR4PM_ERR_INVALID;
    }
    if (n_rows == 0) return GR4PM_OK;
    LineArgs a = {};
    bool any = false;
    for (size_t r = 0; r < n_rows; ++r) {
        const uint64_t n = lengths ? lengths[r] : n_cols;
        if (n > n_cols) {
            set_error("line_spectrum: lengths[%zu] is %llu, a row has %zu columns", r, static_cast<unsigned long long>(n), n_cols);
            return GR4PM_ERR_INVALID;
        }
        if (n > hl::kLineMaxItems) {
            set_error("line_spectrum: lengths[%zu] is %llu, at most 2^40", r, static_cast<unsigned long long>(n));
            return GR4PM_ERR_OVERFLOW;
        }
        a.lengths[r] = n;
        any = any || n != 0;
    }
    if (n_rows > 1 && stride < n_cols) {
        set_error("line_spectrum: a stride of %zu items for rows of %zu columns", stride, n_cols);
        return GR4PM_ERR_INVALID;
    }
    if (any && !x) {
        set_error("line_spectrum: no input array");
        return GR4PM_ERR_INVALID;
    }
    if (!out) {
        set_error("line_spectrum: no output array");
        return GR4PM_ERR_INVALID;
    }
    const hl::LinePlan plan = hl::line_plan(a.lengths, n_rows, h->hop, statistic == GR4PM_LINE_ENVELOPE);
    std::copy(plan.run_start, plan.run_start + hl::kLineMaxRows + 1, a.run_start);
    a.x = reinterpret_cast<const cf*>(x), a.stride = stride, a.gains = gains;
    a.window = h->tf.d_window.p, a.tT = h->tf.d_tT.p, a.cc = h->tf.d_cc.p;
    a.part = h->d_part.p, a.acc = h->d_acc.p, a.out = out, a.window_power = h->tf.window_power;
    a.R = static_cast<uint32_t>(n_rows), a.hop = static_cast<uint32_t>(h->hop);
    const uint64_t total = plan.run_start[n_rows];
    if (statistic == GR4PM_LINE_ENVELOPE)
        launch_all<GR4PM_LINE_ENVELOPE>(h, a, total);
    else if (statistic == GR4PM_LINE_SQUARE)
        launch_all<GR4PM_LINE_SQUARE>(h, a, total);
    else
        launch_all<GR4PM_LINE_FOURTH>(h, a, total);
    GR4PM_HIP_TRY(hipGetLastError());
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_find_line(const double* spectrum, size_t n, const gr4pm_line_params* p, gr4pm_line* out)
try {
    if (!spectrum || !p || !out) return GR4PM_ERR_INVALID;
    if (!hl::line_window_valid(n, p->first_bin, p->n_bins, p->guard_bins)) {
        set_error("find_line: a window of %llu bins from bin %llu with %llu guard bins on a circle of %zu: need first_bin < n "
                  "and 2 guard_bins + 3 <= n_bins <= n",
                  static_cast<unsigned long long>(p->n_bins), static_cast<unsigned long long>(p->first_bin),
                  static_cast<unsigned long long>(p->guard_bins), n);
        return GR4PM_ERR_INVALID;
    }
    *out = hl::find_line(spectrum, n, p->first_bin, p->n_bins, p->guard_bins);
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_simplest_ratio(double value, double rel_tol, uint32_t max_num, uint32_t max_den, uint32_t* num, uint32_t* den)
try {
    if (!num || !den) return GR4PM_ERR_INVALID;
    *num = 0, *den = 0;
    if (!hl::ratio_arguments_valid(value, rel_tol, max_num, max_den)) {
        set_error("simplest_ratio: need a finite value > 0, 0 <= rel_tol < 1 and maxima of at least 1");
        return GR4PM_ERR_INVALID;
    }
    if (!hl::simplest_ratio(value, rel_tol, max_num, max_den, num, den)) {
        set_error("simplest_ratio: no fraction within %g of %.17g has a numerator <= %u and a denominator <= %u", rel_tol, value,
                  max_num, max_den);
        return GR4PM_ERR_INVALID;
    }
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

} // extern "C"
