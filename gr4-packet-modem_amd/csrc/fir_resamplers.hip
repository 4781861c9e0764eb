// fir_resamplers.hip -- InterpolatingFirFilter and PfbArbResampler.  The resampler's phase accumulator is float / double
// rounding dependent: one lane replays it serially and leaves checkpoints, the inner products run in parallel.
// (Conventions of the stream blocks, and the FIR family's item helpers: stream_blocks.hpp.)
#include "stream_blocks.hpp"

namespace gr4pm {
namespace {

// InterpolatingFirFilter::processBulk (interpolating_fir_filter.hpp:93-99): taps laid out
// [arm][arm_stride]; out[n*L + j] = sum_m arm_j[m] * x[n - m], m ascending, acc from 0.
// One thread per INPUT item: a workgroup stages its 256 items and the arm_stride - 1 before them in LDS once
// (coalesced), every thread then forms its L outputs from LDS (neighbouring lanes read neighbouring items, the taps
// are broadcast reads) and writes them as one contiguous run of L items.  Round 1 had one thread per OUTPUT: every
// item was fetched L * arm length times through L1 and every output paid two 64-bit divisions (542 us per 2^24
// symbols in, 2^26 samples out; this form: see HISTORY.md section 5).
constexpr unsigned kFirItems = 256;
inline size_t interp_fir_smem(size_t L, size_t arm_stride, size_t item_size)
{
    return ((kFirItems + arm_stride) * item_size + 15) / 16 * 16 + L * arm_stride * sizeof(float) + L * sizeof(unsigned);
}
template <typename T>
__global__ __launch_bounds__(kFirItems) void k_interp_fir(const T* __restrict__ in, const T* __restrict__ carry,
                                                          unsigned cap, const float* __restrict__ taps,
                                                          const unsigned* __restrict__ arm_len, unsigned arm_stride,
                                                          unsigned L, size_t n_in, T* __restrict__ out)
{
    // LDS: the item tile first (16-byte aligned whatever L * arm_stride is: complex items are read and written as
    // 64-bit words), then the taps, then the arm lengths; interp_fir_smem() is the host's copy of this layout
    extern __shared__ float4 s_fir[];
    T* tile = reinterpret_cast<T*>(s_fir); // tile[i] = x[n0 - (arm_stride - 1) + i]
    float* s_taps = reinterpret_cast<float*>(s_fir + ((kFirItems + arm_stride) * sizeof(T) + 15u) / 16u);
    unsigned* s_len = reinterpret_cast<unsigned*>(s_taps + L * arm_stride);
    for (unsigned i = threadIdx.x; i < L * arm_stride; i += kFirItems) s_taps[i] = taps[i];
    for (unsigned i = threadIdx.x; i < L; i += kFirItems) s_len[i] = arm_len[i];
    const unsigned hist = arm_stride - 1;
    for (size_t n0 = static_cast<size_t>(blockIdx.x) * kFirItems; n0 < n_in; n0 += static_cast<size_t>(gridDim.x) * kFirItems) {
        __syncthreads(); // taps staged / the tile of the round before is no longer read
        const unsigned count = static_cast<unsigned>(min(static_cast<size_t>(kFirItems), n_in - n0));
        for (unsigned i = threadIdx.x; i < count + hist; i += kFirItems)
            tile[i] = item_at(in, carry, cap, static_cast<long long>(n0) + i - hist);
        __syncthreads();
        if (threadIdx.x < count && L == 4) {
            // the usual interpolation: every item is read from LDS once for the four arms, the four outputs leave as
            // one 32-byte (complex) or 16-byte (float) run.  Per arm the sum still runs over m ascending.
            const T* x = tile + hist + threadIdx.x;
            const unsigned l0 = s_len[0], l1 = s_len[1], l2 = s_len[2], l3 = s_len[3];
            T a0 = zero_item(T{}), a1 = a0, a2 = a0, a3 = a0;
            for (unsigned m = 0; m < arm_stride; ++m) {
                const T v = *(x - m);
                if (m < l0) a0 = mac(a0, s_taps[m], v);
                if (m < l1) a1 = mac(a1, s_taps[arm_stride + m], v);
                if (m < l2) a2 = mac(a2, s_taps[2 * arm_stride + m], v);
                if (m < l3) a3 = mac(a3, s_taps[3 * arm_stride + m], v);
            }
            T* o = out + (n0 + threadIdx.x) * 4;
            if constexpr (sizeof(T) == sizeof(cf)) {
                if ((reinterpret_cast<uintptr_t>(out) & 15u) == 0) { // two 16-byte stores per lane
                    float4* o4 = reinterpret_cast<float4*>(o);
                    o4[0] = make_float4(a0.x, a0.y, a1.x, a1.y);
                    o4[1] = make_float4(a2.x, a2.y, a3.x, a3.y);
                } else {
                    o[0] = a0, o[1] = a1, o[2] = a2, o[3] = a3;
                }
            } else {
                o[0] = a0, o[1] = a1, o[2] = a2, o[3] = a3;
            }
        } else if (threadIdx.x < count) {
            const T* x = tile + hist + threadIdx.x; // x[-m] = item n - m
            T* o = out + (n0 + threadIdx.x) * L;
            for (unsigned j = 0; j < L; ++j) {
                const float* arm = s_taps + j * arm_stride;
                const unsigned len = s_len[j];
                T acc = zero_item(T{});
                for (unsigned m = 0; m < len; ++m) acc = mac(acc, arm[m], *(x - m));
                o[j] = acc;
            }
        }
    }
}

// PfbArbResampler (pfb_arb_resampler.hpp:134-167).  The accumulator recurrence decides which
// input and which arm every output uses; it is float/double rounding dependent, so one lane
// replays it serially and writes a plan; the two inner products per output run in parallel.
struct ArbState {
    unsigned long long last_filter;
    double phase_acc_d;
    float phase_acc_f;
    unsigned produced;
    unsigned long long consumed;
};
// The serial lane keeps to the recurrence itself and leaves a checkpoint of its state every kArbChunk outputs (round 1
// wrote three plan arrays entry by entry from that one lane: 147 ns per output, 6.8 Msamples/s); the filter kernel's
// lanes replay at most kArbChunk - 1 steps from their chunk's checkpoint -- the same operations in the same order, so
// the same (input index, arm, phase) as the serial walk -- and go on to their two inner products.
constexpr unsigned kArbChunk = 64;
template <typename TRate>
struct ArbCk {
    unsigned ii;          // inputs consumed when output k * kArbChunk is formed
    unsigned last_filter; // < filter_size there
    TRate phase_acc;
    unsigned pad[sizeof(TRate) == 8 ? 2 : 3];
};
// One pass of the reference loop between two outputs that both exist: the update of pfb_arb_resampler.hpp:161-166, then
// the input items of :135-138.  With last_filter < filter_size before, decim_rate = q0 filter_size + r0 and wrap <= 1
// the walk "while (last_filter >= filter_size) { ++ii; last_filter -= filter_size; }" takes q0 or q0 + 1 items:
// no loop, no division, 32-bit integers -- the same values as the walk.
template <typename TRate>
__device__ __forceinline__ void arb_step(unsigned& ii, unsigned& last_filter, TRate& phase_acc, unsigned filter_size,
                                         unsigned q0, unsigned r0, TRate filt_rate)
{
    phase_acc += filt_rate;
    const bool wrap = phase_acc > TRate{ 1 };
    phase_acc = wrap ? phase_acc - TRate{ 1 } : phase_acc;
    const unsigned t = last_filter + r0 + (wrap ? 1u : 0u);
    const bool c = t >= filter_size;
    ii += q0 + (c ? 1u : 0u);
    last_filter = c ? t - filter_size : t;
}
// kArbChunk steps of the phase accumulator (see k_arb_plan); eight steps per asm statement (hipcc pads register
// overlaps between statements)
__device__ __forceinline__ void arb_phase_chunk(double& acc, double rate)
{
    const double K = 0x1p1000;
    double t, m;
#pragma unroll
    for (unsigned k = 0; k < kArbChunk; k += 8)
        asm volatile("v_add_f64 %1, %0, %3\n\tv_fma_f64 %2, %1, %4, -%4 clamp\n\tv_add_f64 %0, %1, -%2\n\t"
                     "v_add_f64 %1, %0, %3\n\tv_fma_f64 %2, %1, %4, -%4 clamp\n\tv_add_f64 %0, %1, -%2\n\t"
                     "v_add_f64 %1, %0, %3\n\tv_fma_f64 %2, %1, %4, -%4 clamp\n\tv_add_f64 %0, %1, -%2\n\t"
                     "v_add_f64 %1, %0, %3\n\tv_fma_f64 %2, %1, %4, -%4 clamp\n\tv_add_f64 %0, %1, -%2\n\t"
                     "v_add_f64 %1, %0, %3\n\tv_fma_f64 %2, %1, %4, -%4 clamp\n\tv_add_f64 %0, %1, -%2\n\t"
                     "v_add_f64 %1, %0, %3\n\tv_fma_f64 %2, %1, %4, -%4 clamp\n\tv_add_f64 %0, %1, -%2\n\t"
                     "v_add_f64 %1, %0, %3\n\tv_fma_f64 %2, %1, %4, -%4 clamp\n\tv_add_f64 %0, %1, -%2\n\t"
                     "v_add_f64 %1, %0, %3\n\tv_fma_f64 %2, %1, %4, -%4 clamp\n\tv_add_f64 %0, %1, -%2"
                     : "+v"(acc), "=&v"(t), "=&v"(m)
                     : "v"(rate), "v"(K));
}
__device__ __forceinline__ void arb_phase_chunk(float& acc, float rate)
{
    const float K = 0x1p100f;
    float t, m;
#pragma unroll
    for (unsigned k = 0; k < kArbChunk; k += 8)
        asm volatile("v_add_f32 %1, %0, %3\n\tv_fma_f32 %2, %1, %4, -%4 clamp\n\tv_sub_f32 %0, %1, %2\n\t"
                     "v_add_f32 %1, %0, %3\n\tv_fma_f32 %2, %1, %4, -%4 clamp\n\tv_sub_f32 %0, %1, %2\n\t"
                     "v_add_f32 %1, %0, %3\n\tv_fma_f32 %2, %1, %4, -%4 clamp\n\tv_sub_f32 %0, %1, %2\n\t"
                     "v_add_f32 %1, %0, %3\n\tv_fma_f32 %2, %1, %4, -%4 clamp\n\tv_sub_f32 %0, %1, %2\n\t"
                     "v_add_f32 %1, %0, %3\n\tv_fma_f32 %2, %1, %4, -%4 clamp\n\tv_sub_f32 %0, %1, %2\n\t"
                     "v_add_f32 %1, %0, %3\n\tv_fma_f32 %2, %1, %4, -%4 clamp\n\tv_sub_f32 %0, %1, %2\n\t"
                     "v_add_f32 %1, %0, %3\n\tv_fma_f32 %2, %1, %4, -%4 clamp\n\tv_sub_f32 %0, %1, %2\n\t"
                     "v_add_f32 %1, %0, %3\n\tv_fma_f32 %2, %1, %4, -%4 clamp\n\tv_sub_f32 %0, %1, %2"
                     : "+v"(acc), "=&v"(t), "=&v"(m)
                     : "v"(rate), "v"(K));
}

template <typename TRate>
__global__ void k_arb_plan(ArbState* __restrict__ st, unsigned n_in, unsigned out_cap, unsigned filter_size,
                           unsigned long long decim_rate, unsigned q0, unsigned r0, TRate filt_rate,
                           ArbCk<TRate>* __restrict__ ck)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    unsigned long long last_filter = st->last_filter;
    TRate phase_acc = sizeof(TRate) == 8 ? static_cast<TRate>(st->phase_acc_d)
                                         : static_cast<TRate>(st->phase_acc_f);
    unsigned ii = 0, oi = 0;
    // first pass of the reference loop (n_in > 0 and out_cap > 0: checked by the caller): the carried last_filter may
    // ask for any number of items
    while (last_filter >= filter_size && ii < n_in) {
        ++ii;
        last_filter -= filter_size;
    }
    if (last_filter < filter_size) {
        unsigned lf = static_cast<unsigned>(last_filter);
        for (;;) { // state: output oi is about to be formed from (ii, lf, phase_acc)
            // whole chunks while neither the input nor the output can end inside one: a checkpoint, then kArbChunk
            // steps of straight-line code (every pass of the reference loop in between finds its loop condition true
            // and its items there); the chain of phase_acc is then all that a step costs
            while ((oi & (kArbChunk - 1)) == 0 && oi + kArbChunk < out_cap &&
                   static_cast<unsigned long long>(ii) + static_cast<unsigned long long>(kArbChunk) * (q0 + 1u) < n_in) {
                ArbCk<TRate> c{};
                c.ii = ii, c.last_filter = lf, c.phase_acc = phase_acc;
                ck[oi / kArbChunk] = c;
                // inside a chunk only phase_acc is a chain: the kArbChunk conditional subtractions of filter_size add up
                // to a division of lf + kArbChunk r0 + (number of wraps) by filter_size (every partial sum stays below
                // 2 filter_size, so the walk subtracts exactly when the running sum passes a multiple)
                // THREE dependent instructions per step, no compare, no select, no counter:
                //   t = phase_acc + filt_rate ; m = clamp(t * K - K) ; phase_acc = t - m
                // with K = 2^1000 (2^100 for float): the fused multiply-add is > 1 for every t > 1 (t - 1 >= 2^-52),
                // <= 0 for every t <= 1, so the [0, 1] clamp of the instruction's output modifier makes m exactly
                // 1.0 or 0.0 -- the reference's `if (phase_acc > 1) phase_acc -= 1` (t - 0.0 == t bit for bit).
                // The number of wraps falls out at the end: start + kArbChunk * filt_rate - end is that integer up
                // to rounding noise of 1e-5 at most.  (Round 2: add, add, compare, two selects + three instructions
                // of counting per step: 28 ns per output; now 3 per step.)
                const TRate start = phase_acc;
                arb_phase_chunk(phase_acc, filt_rate);
                const unsigned wraps = static_cast<unsigned>(
                    __double2ll_rn(static_cast<double>(start) + static_cast<double>(kArbChunk) * static_cast<double>(filt_rate) -
                                   static_cast<double>(phase_acc)));
                const unsigned long long sum = static_cast<unsigned long long>(lf) + static_cast<unsigned long long>(kArbChunk) * r0 + wraps;
                const unsigned long long sub = sum / filter_size;
                lf = static_cast<unsigned>(sum - sub * filter_size);
                ii += kArbChunk * q0 + static_cast<unsigned>(sub);
                oi += kArbChunk;
            }
            if ((oi & (kArbChunk - 1)) == 0) {
                ArbCk<TRate> c{};
                c.ii = ii, c.last_filter = lf, c.phase_acc = phase_acc;
                ck[oi / kArbChunk] = c;
            }
            ++oi;
            if (ii < n_in && oi < out_cap) { // the reference's loop condition for the next pass
                const unsigned need = q0 + ((lf + r0 + 1u >= filter_size) ? 1u : 0u); // at most this many items
                if (ii + need <= n_in) {
                    arb_step(ii, lf, phase_acc, filter_size, q0, r0, filt_rate);
                    continue;
                }
            }
            // last pass: the update, then -- if the loop goes on at all -- the walk over what is left of the input
            phase_acc += filt_rate;
            last_filter = static_cast<unsigned long long>(lf) + decim_rate;
            if (phase_acc > TRate{ 1 }) {
                phase_acc -= TRate{ 1 };
                ++last_filter;
            }
            if (!(ii < n_in && oi < out_cap)) break;
            while (last_filter >= filter_size && ii < n_in) {
                ++ii;
                last_filter -= filter_size;
            }
            if (last_filter >= filter_size) break;
            lf = static_cast<unsigned>(last_filter); // the items sufficed after all (need was the upper bound)
        }
    }
    st->last_filter = last_filter;
    st->phase_acc_d = static_cast<double>(phase_acc);
    st->phase_acc_f = static_cast<float>(phase_acc);
    st->produced = oi;
    st->consumed = ii;
}
template <typename TRate>
__global__ void k_arb_filter(const cf* __restrict__ in, const cf* __restrict__ carry, unsigned cap,
                             const float* __restrict__ taps, const float* __restrict__ diff_taps,
                             unsigned arm_size, const ArbState* __restrict__ st, const ArbCk<TRate>* __restrict__ ck,
                             unsigned filter_size, unsigned q0, unsigned r0, TRate filt_rate, cf* __restrict__ out)
{
    const unsigned n_out = st->produced;
    for (unsigned o = blockIdx.x * blockDim.x + threadIdx.x; o < n_out; o += gridDim.x * blockDim.x) {
        const ArbCk<TRate> c = ck[o / kArbChunk];
        unsigned ii = c.ii, last_filter = c.last_filter;
        TRate phase_acc = c.phase_acc;
        for (unsigned r = o % kArbChunk; r > 0; --r) arb_step(ii, last_filter, phase_acc, filter_size, q0, r0, filt_rate);
        const long long idx = static_cast<long long>(ii) - 1;
        const float* arm = taps + static_cast<size_t>(last_filter) * arm_size;
        const float* darm = diff_taps + static_cast<size_t>(last_filter) * arm_size;
        cf filt = { 0.f, 0.f }, diff = { 0.f, 0.f };
        for (unsigned m = 0; m < arm_size; ++m) filt = mac(filt, arm[m], item_at(in, carry, cap, idx - m));
        for (unsigned m = 0; m < arm_size; ++m) diff = mac(diff, darm[m], item_at(in, carry, cap, idx - m));
        out[o] = cadd(filt, fmulc(static_cast<float>(phase_acc), diff)); // :153-160
    }
}
// history after the call: last cap items of (carry ++ in[0..consumed))
__global__ void k_arb_update_hist(const cf* __restrict__ in, const cf* __restrict__ carry,
                                  cf* __restrict__ carry_next, unsigned cap,
                                  const ArbState* __restrict__ st)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap) return;
    carry_next[i] = item_at(in, carry, cap, static_cast<long long>(st->consumed) - cap + i);
}

} // namespace
} // namespace gr4pm

using namespace gr4pm;

// ------------------------------------------------------------------ InterpolatingFirFilter
struct gr4pm_interp_fir {
    size_t L, n_taps;
    int item_kind;
    unsigned cap, arm_stride;
    hipStream_t stream;
    DevBuf<float> taps;
    DevBuf<unsigned> arm_len;
    DevBuf<char> carry[2];
    int cur = 0;
};

template <typename T>
static gr4pm_status interp_fir_run(gr4pm_interp_fir* h, const void* in, size_t n_in, void* out)
{
    hipStream_t s = h->stream;
    const T* carry = reinterpret_cast<const T*>(h->carry[h->cur].p);
    T* carry_next = reinterpret_cast<T*>(h->carry[h->cur ^ 1].p);
    const size_t smem = interp_fir_smem(h->L, h->arm_stride, sizeof(T));
    if (smem > kFirMaxSmem) {
        set_error("InterpolatingFirFilter: %zu taps x %zu arms need %zu bytes of LDS per workgroup (limit %zu)",
                  static_cast<size_t>(h->arm_stride), static_cast<size_t>(h->L), smem, kFirMaxSmem);
        return GR4PM_ERR_INVALID;
    }
    if (smem > 48 * 1024) // beyond the default dynamic-LDS window
        GR4PM_TRY(raise_dynamic_lds({ reinterpret_cast<const void*>(&k_interp_fir<T>) }, smem, "interp_fir"));
    hipLaunchKernelGGL(k_interp_fir<T>, dim3(grid_for(n_in, kFirItems, 65536)), dim3(kFirItems), smem, s,
                       static_cast<const T*>(in), carry, h->cap, h->taps.p, h->arm_len.p, h->arm_stride,
                       static_cast<unsigned>(h->L), n_in, static_cast<T*>(out));
    hipLaunchKernelGGL(k_update_hist<T>, dim3((h->cap + 63) / 64), dim3(64), 0, s, static_cast<const T*>(in),
                       carry, carry_next, h->cap, n_in);
    GR4PM_HIP_TRY(hipGetLastError());
    GR4PM_HIP_TRY(hipStreamSynchronize(s));
    h->cur ^= 1;
    return GR4PM_OK;
}

extern "C" {

gr4pm_status gr4pm_interp_fir_create(const gr4pm_interp_fir_params* p, gr4pm_interp_fir** out)
try {
    if (!p || !out || !p->taps) return GR4PM_ERR_INVALID;
    *out = nullptr;
    if (p->interpolation == 0) { // interpolating_fir_filter.hpp:45-47
        set_error("interpolation cannot be zero");
        return GR4PM_ERR_INVALID;
    }
    GR4PM_TRY(require_device());
    std::unique_ptr<gr4pm_interp_fir> h(new (std::nothrow) gr4pm_interp_fir);
    if (!h) return GR4PM_ERR_NOMEM;
    h->L = p->interpolation;
    h->n_taps = p->n_taps;
    h->item_kind = p->item_kind;
    h->stream = static_cast<hipStream_t>(p->stream);
    const size_t arm_max = (p->n_taps + h->L - 1) / h->L;
    h->arm_stride = static_cast<unsigned>(std::max<size_t>(arm_max, 1));
    h->cap = static_cast<unsigned>(bit_ceil_sz(std::max<size_t>(arm_max, 1))); // :63-64
    std::vector<float> taps(h->L * h->arm_stride, 0.0f);
    std::vector<unsigned> arm_len(h->L, 0);
    for (size_t j = 0; j < h->L; ++j)
        for (size_t k = j; k < p->n_taps; k += h->L) taps[j * h->arm_stride + arm_len[j]++] = p->taps[k]; // :54-60
    const size_t isz = p->item_kind == 0 ? sizeof(cf) : sizeof(float);
    GR4PM_TRY(h->taps.alloc(taps.size()));
    GR4PM_TRY(h->arm_len.alloc(arm_len.size()));
    for (auto& c : h->carry) {
        GR4PM_TRY(c.alloc(h->cap * isz));
        GR4PM_TRY(c.zero(h->stream));
    }
    GR4PM_TRY(h->taps.upload(taps.data(), taps.size(), h->stream));
    GR4PM_TRY(h->arm_len.upload(arm_len.data(), arm_len.size(), h->stream));
    return finish_create(h, out, "interp_fir");
}
GR4PM_ABI_CATCH
void gr4pm_interp_fir_destroy(gr4pm_interp_fir* h)
try {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    delete h;
}
GR4PM_ABI_CATCH_VOID
gr4pm_status gr4pm_interp_fir_reset(gr4pm_interp_fir* h)
try {
    if (!h) return GR4PM_ERR_INVALID;
    for (int i = 0; i < 2; ++i) GR4PM_TRY(h->carry[i].zero(h->stream));
    GR4PM_HIP_TRY(hipStreamSynchronize(h->stream));
    return GR4PM_OK;
}
GR4PM_ABI_CATCH
gr4pm_status gr4pm_interp_fir_process(gr4pm_interp_fir* h, const void* in, size_t n_in, void* out)
try {
    if (!h) return GR4PM_ERR_INVALID;
    if (n_in == 0) return GR4PM_OK;
    if (!in || !out) {
        set_error("null sample pointer");
        return GR4PM_ERR_INVALID;
    }
    return h->item_kind == 0 ? interp_fir_run<cf>(h, in, n_in, out) : interp_fir_run<float>(h, in, n_in, out);
}
GR4PM_ABI_CATCH

} // extern "C"

// ------------------------------------------------------------------ PfbArbResampler
struct gr4pm_pfb_arb_resampler {
    size_t filter_size, arm_size, n_taps;
    int rate_is_double;
    unsigned long long decim_rate;
    double filt_rate_d;
    float filt_rate_f;
    unsigned cap, plan_cap = 0;
    hipStream_t stream;
    DevBuf<float> taps, diff_taps;
    DevBuf<cf> carry[2];
    DevBuf<ArbState> st;
    DevBuf<char> plan_ck; // ArbCk<TRate> per kArbChunk outputs
    PinnedBuf<ArbState> st_host;
    int cur = 0;
};

static gr4pm_status arb_reset_impl(gr4pm_pfb_arb_resampler* h)
{
    ArbState st{};
    st.last_filter = (h->n_taps / 2) % h->filter_size; // pfb_arb_resampler.hpp:119
    st.phase_acc_d = 0.0;                              // :118
    st.phase_acc_f = 0.0f;
    *h->st_host.p = st;
    GR4PM_HIP_TRY(hipMemcpyAsync(h->st.p, h->st_host.p, sizeof(ArbState), hipMemcpyHostToDevice, h->stream));
    for (int i = 0; i < 2; ++i) GR4PM_TRY(h->carry[i].zero(h->stream));
    GR4PM_HIP_TRY(hipStreamSynchronize(h->stream));
    return GR4PM_OK;
}

extern "C" {

gr4pm_status gr4pm_pfb_arb_resampler_create(const gr4pm_pfb_arb_resampler_params* p,
                                            gr4pm_pfb_arb_resampler** out)
try {
    if (!p || !out) return GR4PM_ERR_INVALID;
    *out = nullptr;
    if (p->filter_size == 0) { // :70-72
        set_error("filter_size cannot be 0");
        return GR4PM_ERR_INVALID;
    }
    if (!p->taps || p->n_taps < 2) {
        set_error("taps required (the default prototype is supplied by the host wrapper)");
        return GR4PM_ERR_INVALID;
    }
    GR4PM_TRY(require_device());
    std::unique_ptr<gr4pm_pfb_arb_resampler> h(new (std::nothrow) gr4pm_pfb_arb_resampler);
    if (!h) return GR4PM_ERR_NOMEM;
    h->filter_size = p->filter_size;
    h->n_taps = p->n_taps;
    h->rate_is_double = p->rate_is_double;
    h->stream = static_cast<hipStream_t>(p->stream);
    h->arm_size = (p->n_taps + p->filter_size - 1) / p->filter_size; // :74
    std::vector<float> taps(h->filter_size * h->arm_size, 0.0f), diff(h->filter_size * h->arm_size, 0.0f);
    for (size_t j = 0; j < h->filter_size; ++j) { // :77-102
        size_t m = 0;
        for (size_t k = j; k < p->n_taps; k += h->filter_size) taps[j * h->arm_size + m++] = p->taps[k];
        m = 0;
        for (size_t k = j; k < p->n_taps - 1; k += h->filter_size)
            diff[j * h->arm_size + m++] = p->taps[k + 1] - p->taps[k];
    }
    h->cap = static_cast<unsigned>(bit_ceil_sz(h->arm_size)); // :105
    if (h->rate_is_double) { // :115-117
        const double fr = static_cast<double>(h->filter_size) / p->rate;
        h->decim_rate = static_cast<unsigned long long>(std::floor(fr));
        h->filt_rate_d = fr - static_cast<double>(h->decim_rate);
        h->filt_rate_f = 0.0f;
    } else {
        const float fr = static_cast<float>(h->filter_size) / static_cast<float>(p->rate);
        h->decim_rate = static_cast<unsigned long long>(std::floor(fr));
        h->filt_rate_f = fr - static_cast<float>(h->decim_rate);
        h->filt_rate_d = 0.0;
    }
    GR4PM_TRY(h->taps.alloc(taps.size()));
    GR4PM_TRY(h->diff_taps.alloc(diff.size()));
    GR4PM_TRY(h->st.alloc(1));
    GR4PM_TRY(h->st_host.alloc(1));
    for (auto& c : h->carry) GR4PM_TRY(c.alloc(h->cap));
    GR4PM_TRY(h->taps.upload(taps.data(), taps.size(), h->stream));
    GR4PM_TRY(h->diff_taps.upload(diff.data(), diff.size(), h->stream));
    GR4PM_HIP_TRY(hipStreamSynchronize(h->stream));
    GR4PM_TRY(arb_reset_impl(h.get()));
    return finish_create(h, out, "pfb_arb_resampler");
}
GR4PM_ABI_CATCH
void gr4pm_pfb_arb_resampler_destroy(gr4pm_pfb_arb_resampler* h)
try {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    delete h;
}
GR4PM_ABI_CATCH_VOID
gr4pm_status gr4pm_pfb_arb_resampler_reset(gr4pm_pfb_arb_resampler* h)
try {
    return h ? arb_reset_impl(h) : GR4PM_ERR_INVALID;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_pfb_arb_resampler_process(gr4pm_pfb_arb_resampler* h, const gr4pm_c64* in, size_t n_in,
                                             gr4pm_c64* out, size_t out_cap, size_t* consumed, size_t* produced)
try {
    if (!h || !consumed || !produced) return GR4PM_ERR_INVALID;
    *consumed = *produced = 0;
    if (n_in == 0 || out_cap == 0) return GR4PM_OK;
    if (!in || !out) {
        set_error("null sample pointer");
        return GR4PM_ERR_INVALID;
    }
    if (out_cap > 0xffffffffull || n_in > 0x7fffffffull) return GR4PM_ERR_INVALID;
    hipStream_t s = h->stream;
    const size_t n_ck = out_cap / kArbChunk + 2;
    if (h->plan_cap < n_ck) {
        GR4PM_TRY(h->plan_ck.alloc(n_ck * 24)); // ArbCk<float> / ArbCk<double>: 24 bytes each
        h->plan_cap = static_cast<unsigned>(n_ck);
    }
    static_assert(sizeof(ArbCk<float>) == 24 && sizeof(ArbCk<double>) == 24, "checkpoint layout");
    const cf* carry = h->carry[h->cur].p;
    const unsigned grid = grid_for(out_cap, 256, 16384);
    const unsigned fs = static_cast<unsigned>(h->filter_size);
    if (h->decim_rate / fs >= (1ull << 30)) {
        // the plan kernels walk the input with 32-bit item counts (q0 items per output, q0 + 1 after a wrap): a rate this
        // small would wrap them where the reference's 64-bit walk (pfb_arb_resampler.hpp:135-138) does not
        set_error("PfbArbResampler: rate too small for the device path (decim_rate / filter_size = %llu >= 2^30)",
                  static_cast<unsigned long long>(h->decim_rate / fs));
        return GR4PM_ERR_INVALID;
    }
    const unsigned q0 = static_cast<unsigned>(h->decim_rate / fs), r0 = static_cast<unsigned>(h->decim_rate % fs);
    if (h->rate_is_double) {
        auto* ck = reinterpret_cast<ArbCk<double>*>(h->plan_ck.p);
        hipLaunchKernelGGL(k_arb_plan<double>, dim3(1), dim3(64), 0, s, h->st.p, static_cast<unsigned>(n_in),
                           static_cast<unsigned>(out_cap), fs, h->decim_rate, q0, r0, h->filt_rate_d, ck);
        hipLaunchKernelGGL(k_arb_filter<double>, dim3(grid), dim3(256), 0, s, reinterpret_cast<const cf*>(in), carry,
                           h->cap, h->taps.p, h->diff_taps.p, static_cast<unsigned>(h->arm_size), h->st.p, ck, fs, q0, r0,
                           h->filt_rate_d, reinterpret_cast<cf*>(out));
    } else {
        auto* ck = reinterpret_cast<ArbCk<float>*>(h->plan_ck.p);
        hipLaunchKernelGGL(k_arb_plan<float>, dim3(1), dim3(64), 0, s, h->st.p, static_cast<unsigned>(n_in),
                           static_cast<unsigned>(out_cap), fs, h->decim_rate, q0, r0, h->filt_rate_f, ck);
        hipLaunchKernelGGL(k_arb_filter<float>, dim3(grid), dim3(256), 0, s, reinterpret_cast<const cf*>(in), carry,
                           h->cap, h->taps.p, h->diff_taps.p, static_cast<unsigned>(h->arm_size), h->st.p, ck, fs, q0, r0,
                           h->filt_rate_f, reinterpret_cast<cf*>(out));
    }
    hipLaunchKernelGGL(k_arb_update_hist, dim3((h->cap + 63) / 64), dim3(64), 0, s,
                       reinterpret_cast<const cf*>(in), carry, h->carry[h->cur ^ 1].p, h->cap, h->st.p);
    GR4PM_HIP_TRY(hipMemcpyAsync(h->st_host.p, h->st.p, sizeof(ArbState), hipMemcpyDeviceToHost, s));
    GR4PM_HIP_TRY(hipGetLastError());
    GR4PM_HIP_TRY(hipStreamSynchronize(s));
    h->cur ^= 1;
    *consumed = h->st_host.p->consumed;
    *produced = h->st_host.p->produced;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

} // extern "C"
