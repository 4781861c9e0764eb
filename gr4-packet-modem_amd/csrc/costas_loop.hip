// costas_loop.hip -- CostasLoop (costas_loop.hpp:92-148): serial per segment (state fully reset by a
// syncword_phase tag, :35-42), one lane per segment; and the probes of its sin/cos and phase wrap.
// (Conventions of the stream blocks: stream_blocks.hpp.)
#include "stream_blocks.hpp"
#include "hostlogic/costas_plan.hpp"

namespace gr4pm {
namespace {

struct CostasState {
    float phase, freq;
};
using hostlogic::CostasSeg; // hostlogic/costas_plan.hpp

// cos/sin of the loop phase, BIT-EXACT with glibc's cosf / sinf / sincosf (what the reference's
// std::cos(float) / std::sin(float) call, costas_loop.hpp:113-115).  glibc >= 2.28 evaluates them in
// double (sysdeps/ieee754/flt-32/s_sinf.c, s_cosf.c, s_sincosf.h: Szabolcs Nagy's routines): the
// quadrant n from x * (2/pi * 2^24) by an integer shift, x - n * (pi/2 as a double), one sine and one
// cosine polynomial in x^2, ONE rounding to float.  MI355X has the FP64 rate to do the same, so the
// loop's local oscillator carries the reference's bits instead of "< 1 ULP" ones.  Pinned against the
// host libm for every float of |x| <= 3.2 (tests/sincosf_glibc_check.c: 0 mismatches, with and
// without FMA contraction) and on the device by test_device_sincosf_is_glibc_bit_exact.
// Valid for |x| < 120 (glibc's reduce_fast range; the loop phase is wrapped to [-pi, pi)).
__device__ __forceinline__ void sincosf_glibc(float y, float* s_out, float* c_out)
{
    const double hpi_inv = 0x1.45F306DC9C883p+23, hpi = 0x1.921FB54442D18p0; // 2/pi * 2^24, pi/2
    const double C0 = 0x1p0, C1 = -0x1.ffffffd0c621cp-2, C2 = 0x1.55553e1068f19p-5, C3 = -0x1.6c087e89a359dp-10,
                 C4 = 0x1.99343027bf8c3p-16, S1 = -0x1.555545995a603p-3, S2 = 0x1.1107605230bc4p-7,
                 S3 = -0x1.994eb3774cf24p-13;
    const double x0 = static_cast<double>(y);
    // reduce_fast (for |y| < pi/4 this yields n = 0 and x = x0: the same as glibc's short path)
    const int n = (static_cast<int>(x0 * hpi_inv) + 0x800000) >> 24;
    const double x = fma(-static_cast<double>(n), hpi, x0);
    const double x2 = x * x;
    // sinf_poly, even n
    const double x3 = x * x2;
    const double s1 = fma(x2, S3, S2);
    const double x7 = x3 * x2;
    const double sp = fma(x7, s1, fma(x3, S1, x));
    // sinf_poly, odd n
    const double x4 = x2 * x2;
    const double c2 = fma(x2, C4, C3);
    const double c1 = fma(x2, C1, C0);
    const double x6 = x4 * x2;
    const double cp = fma(x6, c2, fma(x4, C2, c1));
    float sn = static_cast<float>(sp), cs = static_cast<float>(cp);
    // Tiny arguments (|y| < 2^-12): glibc returns y and 1.0f without evaluating anything.  The polynomials give the same
    // bits by themselves -- cos: x^2 |C1| < 2^-25, so cp > 1 - 2^-25 rounds to 1.0f; sin: sp = x (1 - d) with d < 2^-26
    // rounds back to y -- except for y = -0.0f, where the odd polynomial's sums produce +0.0.  The sign of the sine
    // polynomial IS the sign of the reduced argument whenever the result is not zero, so copying x's sign bit into sn
    // (one v_bfi_b32, no compare, no select) leaves every other value alone and restores the signed zero
    // (tests/sincosf_glibc_check.c and test_device_sincosf_is_glibc_bit_exact sweep it).
    // v_bitop3_b32 (gfx950): any function of three words in one instruction; 0xca = (a & b) | (~a & c), 0x78 = a ^ (b & c)
    const unsigned sb = __builtin_amdgcn_bitop3_b32(0x7fffffffu, __float_as_uint(sn), static_cast<unsigned>(__double2hiint(x)), 0xca);
    const unsigned cb = __float_as_uint(cs);
    // quadrant: sign[n & 3] on the sine argument (an odd polynomial: exact negation), second table =
    // cosine polynomial negated when n & 2; odd n swaps the two.  Bit arithmetic on a 0 / ~0 mask instead of
    // compare + select: a v_cmp result needs wait states before the v_cndmask that reads it, and this chain has
    // nothing to fill them with.  Eight instructions for tiny / swap / signs together (round 2: fifteen + 4 s_nop).
    const unsigned swap = static_cast<unsigned>(__builtin_amdgcn_sbfe(n, 0, 1)); // 0 or ~0
    const unsigned s0 = __builtin_amdgcn_bitop3_b32(swap, cb, sb, 0xca);
    const unsigned c0 = __builtin_amdgcn_bitop3_b32(swap, sb, cb, 0xca);
    const unsigned q = static_cast<unsigned>(n) << 30; // bit 31 = n & 2, bit 30 = n & 1
    *s_out = __uint_as_float(__builtin_amdgcn_bitop3_b32(s0, q, 0x80000000u, 0x78));
    *c_out = __uint_as_float(__builtin_amdgcn_bitop3_b32(c0, q + 0x40000000u, 0x80000000u, 0x78));
}

// costas_loop.hpp:141-145: phase >= pi ? phase - 2 pi : (phase < -pi ? phase + 2 pi : phase), without compares:
//   up   = clamp(phase * K - below(pi) * K)   1.0f for phase > below(pi) <=> phase >= pi (below = the next float down),
//   down = clamp(-phase * K - pi * K)         1.0f for phase < -pi, else 0.0f (K = 2^100: the smallest positive
//                                             difference, one ulp of pi = 2^-22, still scales past 1)
//   phase = fma(up - down, -2 pi, phase)
// up - down is 1, -1 or +0 (at most one of the two is 1): fma(+-1, -2 pi, phase) is the reference's single rounding
// of phase -+ 2 pi, and fma(+0, -2 pi, phase) = -0 + phase is phase bit for bit, the signed zeros included (a product
// of +0 with a POSITIVE constant would turn a phase of -0.0 into +0.0).  Four instructions, no VCC round trip (was
// six + wait states).
__device__ __forceinline__ float costas_wrap(float phase, float pi_f)
{
    const float K = 0x1p100f, two_pi = 2.0f * pi_f;
    const float pi_below = __uint_as_float(__float_as_uint(pi_f) - 1u);
    float up, down;
    asm("v_fma_f32 %0, %2, %3, -%4 clamp\n\t"
        "v_fma_f32 %1, -%2, %3, -%5 clamp"
        : "=&v"(up), "=&v"(down)
        : "v"(phase), "v"(K), "v"(pi_below * K), "v"(pi_f * K));
    return __builtin_fmaf(up - down, -two_pi, phase);
}

// one PLL iteration, costas_loop.hpp:112-146.  Everything is straight-line code without exec-mask branches; the phase
// wrap and sincosf's quadrant logic also without compares (round 3; the QPSK error term keeps its two selects): the
// chain of dependent operations of one iteration is the whole cost of the block.
template <int CONSTELLATION>
__device__ __forceinline__ cf costas_step(cf x, float& phase, float& freq, float k1, float k2)
{
    const float pi_f = 3.14159265358979323846f;
    float sn, cs;
#ifdef GR4PM_COSTAS_HW_SINCOS
    sn = __sinf(phase);
    cs = __cosf(phase);
#else
    sincosf_glibc(phase, &sn, &cs);
#endif
    const cf lo = { cs, -sn }; // :114-115
    const cf z = cmul(x, lo);
    float error;
    if constexpr (CONSTELLATION == 0) error = z.y;
    else if constexpr (CONSTELLATION == 1) error = z.x * z.y;
    else error = (z.x > 0 ? z.y : -z.y) + (z.y > 0 ? -z.x : z.x);
    freq += k2 * error;
    phase += k1 * error + freq;
    phase = costas_wrap(phase, pi_f);
    return z;
}

// The PLL over `len` items starting at item `base` (one lane).  Lanes walk different
// segments, so every load instruction touches 64 different cache lines: whole 128-byte
// lines are loaded with 16-byte instructions, one chunk (16 symbols) ahead of the PLL.
// KV: float4 per prefetched chunk.  8 = whole 128-byte lines, the fastest loop by itself; 2 keeps
// k_costas under 48 VGPRs, which is what a SIMD has left beside two correlator waves
// (gr4pm_costas_loop_set_small_footprint; the pipelined receiver asks for it): the kernel alone then
// takes 1.06 instead of 0.63 ms per 2^26 samples, but the pipelined front end gains 2.7 % (the
// stage has the time, the correlator gets its slots back).
template <int CONSTELLATION, int KV = 8>
__device__ __forceinline__ void costas_run(const cf* __restrict__ in, cf* __restrict__ out, size_t base,
                                           unsigned len, float& phase, float& freq, float k1, float k2)
{
    auto step = [&](cf x) -> cf { return costas_step<CONSTELLATION>(x, phase, freq, k1, k2); };
    constexpr int kV = KV;           // float4 per chunk
    constexpr unsigned kC = 2 * kV;  // symbols per chunk
    unsigned j = 0;
    if (((base + j) & 1) && j < len) { // align to 16 bytes
        out[base + j] = step(in[base + j]);
        ++j;
    }
    // two register sets: while the PLL walks one chunk, the loads of the next one are in flight
    const unsigned n_chunks = (len - j) / kC;
    if (n_chunks > 0) {
        const float4* ip = reinterpret_cast<const float4*>(in + base + j);
        float4* op = reinterpret_cast<float4*>(out + base + j);
        float4 a[kV], b[kV];
        auto load = [&](float4(&v)[kV], unsigned c) {
            const float4* p = ip + static_cast<size_t>(min(c, n_chunks - 1)) * kV; // clamped: no branch
#pragma unroll
            for (int u = 0; u < kV; ++u) v[u] = p[u];
            // keep the loads up here: hipcc otherwise sinks them to their first use, or lets the
            // PLL arithmetic overtake them.  The empty asm orders the loads (memory clobber) and
            // makes the PLL state, where every chain of arithmetic starts, depend on it.
            asm volatile("" : "+v"(phase), "+v"(freq) : : "memory");
        };
        auto run = [&](float4(&v)[kV], unsigned c) {
#pragma unroll
            for (int u = 0; u < kV; ++u) {
                const cf z0 = step(cf{ v[u].x, v[u].y });
                const cf z1 = step(cf{ v[u].z, v[u].w });
                v[u] = make_float4(z0.x, z0.y, z1.x, z1.y);
            }
            float4* q = op + static_cast<size_t>(c) * kV;
#pragma unroll
            for (int u = 0; u < kV; ++u) q[u] = v[u];
        };
        load(a, 0);
        unsigned c = 0;
        for (; c + 2 <= n_chunks; c += 2) {
            load(b, c + 1);
            run(a, c);
            load(a, c + 2);
            run(b, c + 1);
        }
        if (c < n_chunks) run(a, c);
        j += n_chunks * kC;
    }
    for (; j < len; ++j) out[base + j] = step(in[base + j]);
}

// One lane per segment (the PLL is serial inside a segment).
template <int CONSTELLATION, int KV = 8>
__global__ void k_costas(const CostasSeg* __restrict__ segs, unsigned n_segs,
                         const CostasState* __restrict__ state, CostasState* __restrict__ state_next,
                         float k1, float k2,
                         const cf* __restrict__ in, cf* __restrict__ out, size_t stride)
{
    const unsigned s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_segs) return;
    __builtin_amdgcn_s_setprio(GR4PM_SERIAL_PRIO); // a few latency-bound waves among throughput kernels
    const CostasSeg g = segs[s];
    float phase, freq;
    if (g.mode == 0) {
        phase = state[g.channel].phase;
        freq = state[g.channel].freq;
    } else {
        phase = g.phase0;
        freq = 0.0f;
    }
    costas_run<CONSTELLATION, KV>(in, out, static_cast<size_t>(g.channel) * stride + g.start, g.len, phase, freq, k1,
                              k2);
    if (g.last) { // ping-pong: another lane may still have to read `state`
        state_next[g.channel].phase = phase;
        state_next[g.channel].freq = freq;
    }
}

// The same kernel held to 32 VGPRs (amdgpu_num_vgpr counts register PAIRS on gfx90a and later: 16 -> 32; hipcc spills
// 26 - 30 dwords, six scratch accesses per four symbols in the loop), which is what a SIMD has left beside two 240-VGPR
// correlator waves: its waves start beside a correlator workgroup instead of waiting for -- and then keeping -- a CU
// of their own.  Slower by itself, +2.5 % for the pipelined receiver (gr4pm_costas_loop_set_small_footprint(h, 2)).
template <int CONSTELLATION, int KV>
__global__ __attribute__((amdgpu_num_vgpr(16))) void k_costas_cap(const CostasSeg* __restrict__ segs, unsigned n_segs,
                                                               const CostasState* __restrict__ state,
                                                               CostasState* __restrict__ state_next, float k1, float k2,
                                                               const cf* __restrict__ in, cf* __restrict__ out,
                                                               size_t stride)
{
    const unsigned s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_segs) return;
    __builtin_amdgcn_s_setprio(GR4PM_SERIAL_PRIO);
    const CostasSeg g = segs[s];
    float phase, freq;
    if (g.mode == 0) {
        phase = state[g.channel].phase;
        freq = state[g.channel].freq;
    } else {
        phase = g.phase0;
        freq = 0.0f;
    }
    costas_run<CONSTELLATION, KV>(in, out, static_cast<size_t>(g.channel) * stride + g.start, g.len, phase, freq, k1, k2);
    if (g.last) {
        state_next[g.channel].phase = phase;
        state_next[g.channel].freq = freq;
    }
}

// Tag-driven settings (gr4pm_costas_loop_process_packets): one lane per chain of pieces (hostlogic/costas_plan.hpp)
using hostlogic::CostasChain;
using hostlogic::CostasPiece;
template <int KV>
__device__ __forceinline__ void costas_chains_body(const CostasChain* __restrict__ chains, unsigned n_chains,
                                                   const CostasPiece* __restrict__ pieces,
                                                   const CostasState* __restrict__ state,
                                                   CostasState* __restrict__ state_next, const cf* __restrict__ in,
                                                   cf* __restrict__ out)
{
    const unsigned s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_chains) return;
    __builtin_amdgcn_s_setprio(GR4PM_SERIAL_PRIO);
    const CostasChain ch = chains[s];
    float phase, freq;
    if (ch.mode == 0) {
        phase = state[0].phase;
        freq = state[0].freq;
    } else {
        phase = ch.phase0;
        freq = 0.0f;
    }
    for (unsigned q = 0; q < ch.n_pieces; ++q) {
        const CostasPiece pc = pieces[ch.piece0 + q];
        const cf* src = in + pc.in_off;
        if (pc.constellation == 0) costas_run<0, KV>(src, out, pc.start, pc.len, phase, freq, pc.k1, pc.k2);
        else if (pc.constellation == 1) costas_run<1, KV>(src, out, pc.start, pc.len, phase, freq, pc.k1, pc.k2);
        else costas_run<2, KV>(src, out, pc.start, pc.len, phase, freq, pc.k1, pc.k2);
    }
    if (ch.last) {
        state_next[0].phase = phase;
        state_next[0].freq = freq;
    }
}
template <int KV>
__global__ void k_costas_chains(const CostasChain* __restrict__ chains, unsigned n_chains,
                                const CostasPiece* __restrict__ pieces, const CostasState* __restrict__ state,
                                CostasState* __restrict__ state_next, const cf* __restrict__ in,
                                cf* __restrict__ out)
{
    costas_chains_body<KV>(chains, n_chains, pieces, state, state_next, in, out);
}
// The same chains held to 32 VGPRs, as k_costas_cap is (round 6): the decode_headers / soft_bits receivers' PLL -- 121
// VGPRs in the form above -- could not start beside a correlator workgroup (2 x 240 of a SIMD's 512 registers): each of
// its one-wave workgroups (one per 64 packets) waited for a compute unit and then kept a correlator workgroup off it for
// as long as a packet's chain takes.
__global__ __attribute__((amdgpu_num_vgpr(16))) void k_costas_chains_cap(const CostasChain* __restrict__ chains, unsigned n_chains,
                                                                      const CostasPiece* __restrict__ pieces,
                                                                      const CostasState* __restrict__ state,
                                                                      CostasState* __restrict__ state_next,
                                                                      const cf* __restrict__ in, cf* __restrict__ out)
{
    costas_chains_body<2>(chains, n_chains, pieces, state, state_next, in, out);
}

__global__ void k_sincosf(const float* __restrict__ x, size_t n, float* __restrict__ sn, float* __restrict__ cs)
{
    const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n) sincosf_glibc(x[i], sn + i, cs + i);
}

__global__ void k_costas_wrap(const float* __restrict__ x, size_t n, float* __restrict__ out)
{
    const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n) out[i] = costas_wrap(x[i], 3.14159265358979323846f);
}

#ifdef GR4PM_EXPERIMENTS
// GR4PM_TIMING_SKIP=costas_fake (timing only; see k_symf_fake, stream_blocks.hip): the life time of a PLL wave, 32 VGPRs
__global__ __launch_bounds__(64) void k_serial_fake(unsigned ticks, float* sink)
{
    const unsigned long long t0 = wall_clock64();
    float x = threadIdx.x;
    while (wall_clock64() - t0 < ticks) {
#pragma unroll
        for (int i = 0; i < 32; ++i) x = __builtin_fmaf(x, 1.0001f, 0.5f);
    }
    if (x == 12345.0f) *sink = x;
}
#endif

} // namespace
} // namespace gr4pm

using namespace gr4pm;

// ------------------------------------------------------------------------ CostasLoop
struct gr4pm_costas_loop : gr4pm::hostlogic::CostasHostState { // the settings and their coefficients: hostlogic/costas_plan.hpp
    size_t n_channels;
    hipStream_t stream;
    DevBuf<CostasState> state; // [2][n_channels], st_cur selects the current half
    int st_cur = 0;
    int small_footprint = 0; // 0: k_costas<C, 8> (112 VGPRs, fastest alone), 1: k_costas<C, 2> (62), 2: k_costas_cap<C, 2> (32)
    DevBuf<CostasSeg> segs;
    DevBuf<CostasChain> chains;
    DevBuf<CostasPiece> pieces;
};
using hostlogic::costas_coeffs;

extern "C" {

gr4pm_status gr4pm_costas_loop_create(const gr4pm_costas_loop_params* p, gr4pm_costas_loop** out)
try {
    if (!p || !out || p->n_channels == 0 || p->constellation < 0 || p->constellation > 2)
        return GR4PM_ERR_INVALID;
    *out = nullptr;
    GR4PM_TRY(require_device());
    std::unique_ptr<gr4pm_costas_loop> h(new (std::nothrow) gr4pm_costas_loop);
    if (!h) return GR4PM_ERR_NOMEM;
    h->loop_bandwidth = p->loop_bandwidth;
    h->constellation = p->constellation;
    h->n_channels = p->n_channels;
    h->stream = static_cast<hipStream_t>(p->stream);
    costas_coeffs(*h);
    GR4PM_TRY(h->state.alloc(2 * h->n_channels));
    GR4PM_TRY(h->state.zero(h->stream));
    // GR4PM_COSTAS_FORM = 0 .. 2: the kernel form every CostasLoop starts with (tests and A/B; same results)
    static const char* form = gr4pm::experiment_env("GR4PM_COSTAS_FORM", false);
    if (form) h->small_footprint = std::min(2, std::max(0, atoi(form)));
    return finish_create(h, out, "costas_loop");
}
GR4PM_ABI_CATCH
void gr4pm_costas_loop_destroy(gr4pm_costas_loop* h)
try {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    delete h;
}
GR4PM_ABI_CATCH_VOID
gr4pm_status gr4pm_costas_loop_reset(gr4pm_costas_loop* h)
try {
    if (!h) return GR4PM_ERR_INVALID;
    GR4PM_TRY(h->state.zero(h->stream));
    GR4PM_HIP_TRY(hipStreamSynchronize(h->stream));
    h->st_cur = 0;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH
void gr4pm_costas_loop_coeffs(const gr4pm_costas_loop* h, float* k1, float* k2)
try {
    *k1 = h->k1;
    *k2 = h->k2;
}
GR4PM_ABI_CATCH_VOID
gr4pm_status gr4pm_costas_loop_set(gr4pm_costas_loop* h, double loop_bandwidth, int constellation)
try {
    if (!h || constellation < 0 || constellation > 2) return GR4PM_ERR_INVALID;
    h->loop_bandwidth = loop_bandwidth;
    h->constellation = constellation;
    costas_coeffs(*h);
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

// n_of(c): items of channel c in this call (channels with 0 items keep their state)
extern "C++" {
template <typename NOf>
static gr4pm_status costas_process_impl(gr4pm_costas_loop* h, const gr4pm_c64* in, size_t stride, NOf n_of,
                                        gr4pm_c64* out, const gr4pm_tag* tags, const uint32_t* tag_channel,
                                        size_t n_tags)
{
    // one lane per segment, the longest ones together (hostlogic::costas_segments)
    static const bool costas_no_sort = gr4pm::experiment_env("GR4PM_COSTAS_NO_SORT", false) != nullptr;
    std::vector<CostasSeg> segs;
    hostlogic::costas_segments(h->n_channels, n_of, tags, tag_channel, n_tags, costas_no_sort, segs);
    hipStream_t s = h->stream;
    GR4PM_TRY(upload_vec(h->segs, segs, s));
    if (timing_skip("seg_stats")) { // GR4PM_TIMING_SKIP=seg_stats: what the serial kernel is given
        size_t longest = 0, total = 0;
        for (const auto& g : segs) longest = std::max<size_t>(longest, g.len), total += g.len;
        fprintf(stderr, "[gr4pm costas] %zu segments, %zu items, longest %zu\n", segs.size(), total, longest);
    }
    static const unsigned wg = gr4pm::experiment_env_wg("GR4PM_COSTAS_WG", 64u, 1u, 1024u);
    const dim3 grid(grid_for(segs.size(), wg)), block(wg);
    const unsigned n_segs = static_cast<unsigned>(segs.size());
    const CostasState* st_in = h->state.p + h->st_cur * h->n_channels;
    CostasState* st_out = h->state.p + (h->st_cur ^ 1) * h->n_channels;
    h->st_cur ^= 1;
    auto launch = [&](auto kernel) {
#ifdef GR4PM_EXPERIMENTS
        if (timing_skip("costas_fake")) { // GR4PM_FAKE=workgroups,ticks(10 ns),bytes of LDS
            unsigned wgs = grid.x, ticks = 83000u, lds = 0u;
            static const char* fake = gr4pm::experiment_env("GR4PM_FAKE", true);
            if (fake) sscanf(fake, "%u,%u,%u", &wgs, &ticks, &lds);
            wgs = std::max(wgs, 1u);
            if (lds > 48 * 1024)
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_serial_fake),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
            hipLaunchKernelGGL(k_serial_fake, dim3(wgs), block, lds, s, ticks, reinterpret_cast<float*>(st_out));
            return;
        }
#endif
        if (timing_skip("costas")) return;
        hipLaunchKernelGGL(kernel, grid, block, 0, s, h->segs.p, n_segs, st_in, st_out, h->k1, h->k2,
                           reinterpret_cast<const cf*>(in), reinterpret_cast<cf*>(out), stride);
    };
    // Form 2 pays when the call is long enough for a correlator launch of the same size to keep the chip busy beside it:
    // a PLL wave lives for one packet's chain however small the call is (0.75 ms in the 112-VGPR form, 1.77 ms in the
    // 32-VGPR form), and with batches of 2^26 samples and less that life, not the correlator, is what the receiver waits
    // for (64 channels x 2^20 samples per batch: 40.8 against 25.5 Gsps sustained).  Below 2^25 symbols: the fast form.
    size_t call_symbols = 0;
    for (const auto& g : segs) call_symbols += g.len;
    static const char* cap_min = gr4pm::experiment_env("GR4PM_COSTAS_CAP_MIN_LOG2", false);
    const size_t cap_from = size_t{ 1 } << (cap_min ? std::min(40, std::max(0, atoi(cap_min))) : 25);
    if (h->small_footprint >= 2 && call_symbols >= cap_from) {
        if (h->constellation == 0) launch(k_costas_cap<0, 2>);
        else if (h->constellation == 1) launch(k_costas_cap<1, 2>);
        else launch(k_costas_cap<2, 2>);
    } else if (h->small_footprint == 1) {
        if (h->constellation == 0) launch(k_costas<0, 2>);
        else if (h->constellation == 1) launch(k_costas<1, 2>);
        else launch(k_costas<2, 2>);
    } else {
        if (h->constellation == 0) launch(k_costas<0, 8>);
        else if (h->constellation == 1) launch(k_costas<1, 8>);
        else launch(k_costas<2, 8>);
    }
    GR4PM_HIP_TRY(hipGetLastError());
    GR4PM_HIP_TRY(final_sync(s));
    return GR4PM_OK;
}
} // extern "C++"

gr4pm_status gr4pm_costas_loop_set_small_footprint(gr4pm_costas_loop* h, int on)
try {
    if (!h) return GR4PM_ERR_INVALID;
    h->small_footprint = on < 0 ? 0 : (on > 2 ? 2 : on);
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_costas_loop_process(gr4pm_costas_loop* h, const gr4pm_c64* in, size_t stride, size_t n,
                                       gr4pm_c64* out, const gr4pm_tag* tags, const uint32_t* tag_channel,
                                       size_t n_tags)
try {
    if (!h) return GR4PM_ERR_INVALID;
    if (n == 0) return GR4PM_OK;
    if (!in || !out) {
        set_error("null sample pointer");
        return GR4PM_ERR_INVALID;
    }
    return costas_process_impl(h, in, stride, [n](size_t) { return n; }, out, tags, tag_channel, n_tags);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_costas_loop_process_ragged(gr4pm_costas_loop* h, const gr4pm_c64* in, size_t stride,
                                              const size_t* n_per_channel, gr4pm_c64* out, const gr4pm_tag* tags,
                                              const uint32_t* tag_channel, size_t n_tags)
try {
    if (!h || !n_per_channel) return GR4PM_ERR_INVALID;
    if (!in || !out) {
        set_error("null sample pointer");
        return GR4PM_ERR_INVALID;
    }
    return costas_process_impl(h, in, stride, [n_per_channel](size_t c) { return n_per_channel[c]; }, out, tags,
                               tag_channel, n_tags);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_costas_loop_process_packets(gr4pm_costas_loop* h, const gr4pm_c64* in, size_t n,
                                               gr4pm_c64* out, const gr4pm_packet_tag* tags, size_t n_tags)
try {
    return gr4pm::costas_loop_process_packets_from(h, in, nullptr, 0, n, out, tags, n_tags);
}
GR4PM_ABI_CATCH

} // extern "C"

// (library-internal: csrc/packet_receiver.hip) gr4pm_costas_loop_process_packets with the gather of the block in front
// folded in (round 6): the loop's input stream is not in memory as such -- item i of it is `in[spans[k].src + (i -
// spans[k].dst)]` for the span that holds i (PayloadMetadataInsert's span table, ascending, covering [0, n)).  Saves that
// block's gather: a read and a write of the whole symbol stream.  spans == nullptr: the stream is `in` itself.
gr4pm_status gr4pm::costas_loop_process_packets_from(gr4pm_costas_loop* h, const gr4pm_c64* in, const hostlogic::CopySpan* spans,
                                                     size_t n_spans, size_t n, gr4pm_c64* out, const gr4pm_packet_tag* tags,
                                                     size_t n_tags)
{
    if (!h) return GR4PM_ERR_INVALID;
    if (h->n_channels != 1) {
        set_error("process_packets needs a single-channel CostasLoop");
        return GR4PM_ERR_INVALID;
    }
    if (n == 0) return GR4PM_OK;
    if (!in || !out) {
        set_error("null sample pointer");
        return GR4PM_ERR_INVALID;
    }
    // (the settings follow the tags inside: a refused call leaves those of the tags in front of the refusal applied)
    std::vector<CostasChain> chains;
    std::vector<CostasPiece> pieces;
    GR4PM_TRY(hostlogic::costas_packet_chains(*h, spans, n_spans, n, tags, n_tags, chains, pieces));
    if (chains.empty()) return GR4PM_OK;
    hipStream_t s = h->stream;
    GR4PM_TRY(upload_vec(h->chains, chains, s));
    GR4PM_TRY(upload_vec(h->pieces, pieces, s));
    if (!timing_skip("costas_chains")) { // (EXPERIMENTS builds: GR4PM_TIMING_SKIP=costas_chains, wrong results)
        // the kernel form as in gr4pm_costas_loop_process: 32 VGPRs beside a correlator launch where the call is long enough
        static const char* cap_min = gr4pm::experiment_env("GR4PM_COSTAS_CAP_MIN_LOG2", false);
        const size_t cap_from = size_t{ 1 } << (cap_min ? std::min(40, std::max(0, atoi(cap_min))) : 25);
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(grid_for(chains.size(), 64)), dim3(64), 0, s, h->chains.p,
                               static_cast<unsigned>(chains.size()), h->pieces.p, h->state.p + h->st_cur,
                               h->state.p + (h->st_cur ^ 1), reinterpret_cast<const cf*>(in), reinterpret_cast<cf*>(out));
        };
        if (h->small_footprint >= 2 && n >= cap_from) launch(k_costas_chains_cap);
        else if (h->small_footprint == 1) launch(k_costas_chains<2>);
        else launch(k_costas_chains<8>);
    }
    h->st_cur ^= 1;
    GR4PM_HIP_TRY(hipGetLastError());
    GR4PM_HIP_TRY(final_sync(s));
    return GR4PM_OK;
}

extern "C" {

gr4pm_status gr4pm_sincosf(const float* x, size_t n, float* sin_out, float* cos_out)
try {
    if (!x || !sin_out || !cos_out) return GR4PM_ERR_INVALID;
    GR4PM_TRY(require_device());
    if (n == 0) return GR4PM_OK;
    hipLaunchKernelGGL(k_sincosf, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, nullptr, x, n, sin_out,
                       cos_out);
    GR4PM_HIP_TRY(hipGetLastError());
    GR4PM_HIP_TRY(hipStreamSynchronize(nullptr));
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_costas_phase_wrap(const float* x, size_t n, float* out)
try {
    if (!x || !out) return GR4PM_ERR_INVALID;
    GR4PM_TRY(require_device());
    if (n == 0) return GR4PM_OK;
    hipLaunchKernelGGL(k_costas_wrap, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, nullptr, x, n, out);
    GR4PM_HIP_TRY(hipGetLastError());
    GR4PM_HIP_TRY(hipStreamSynchronize(nullptr));
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

} // extern "C"
