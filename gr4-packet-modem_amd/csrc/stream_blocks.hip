// stream_blocks.hip -- what is left of it: the symbol filter's unit (to be renamed symbol_filter.hip).  SymbolFilter
// (symbol_filter.hpp:208-214): y = scale * sum_m arm[m] * x[idx - m], and its form fused with CoarseFrequencyCorrection (the
// rotation is applied while the filter stages its input, from the plan of rotator.hip).  (Conventions: stream_blocks.hpp.)
#include "rotator.hpp"
#include "hostlogic/symbol_filter_replay.hpp"

namespace gr4pm {
namespace {

// x[t] *= e_t for the eight items of a checkpoint chunk, e_(t+1) = e_t * inc in between (coarse_frequency_correction.hpp:
// 87, rotator.hpp:58-59): cmul_pk's three packed instructions per product, all 45 in ONE statement -- between separate
// asm statements hipcc pads every dependent packed pair with an s_nop (21 of them in this chain).
__device__ __forceinline__ void rot8_pk(cf (&x)[kRotChunk], cf e, cf inc)
{
    static_assert(kRotChunk == 8, "eight items below");
    cf a, b;
#define GR4PM_X(n)                                                          \
    "v_pk_mul_f32 %[a], %[x" #n "], %[e] op_sel_hi:[0,1]\n"                 \
    "v_pk_mul_f32 %[b], %[x" #n "], %[e] op_sel:[1,1] op_sel_hi:[1,0]\n"    \
    "v_pk_add_f32 %[x" #n "], %[a], %[b] neg_lo:[0,1] neg_hi:[0,0]\n"
#define GR4PM_E                                                             \
    "v_pk_mul_f32 %[a], %[e], %[i] op_sel_hi:[0,1]\n"                       \
    "v_pk_mul_f32 %[b], %[e], %[i] op_sel:[1,1] op_sel_hi:[1,0]\n"          \
    "v_pk_add_f32 %[e], %[a], %[b] neg_lo:[0,1] neg_hi:[0,0]\n"
    asm(GR4PM_X(0) GR4PM_E GR4PM_X(1) GR4PM_E GR4PM_X(2) GR4PM_E GR4PM_X(3) GR4PM_E GR4PM_X(4) GR4PM_E GR4PM_X(5) GR4PM_E
            GR4PM_X(6) GR4PM_E GR4PM_X(7)
        : [x0] "+v"(x[0]), [x1] "+v"(x[1]), [x2] "+v"(x[2]), [x3] "+v"(x[3]), [x4] "+v"(x[4]), [x5] "+v"(x[5]),
          [x6] "+v"(x[6]), [x7] "+v"(x[7]), [e] "+v"(e), [a] "=&v"(a), [b] "=&v"(b)
        : [i] "v"(inc));
#undef GR4PM_X
#undef GR4PM_E
}

// SymbolFilter (symbol_filter.hpp:208-214): y = scale * sum_m arm[m] * x[idx - m]
using hostlogic::SymRun; // hostlogic/symbol_filter_replay.hpp
#ifndef GR4PM_SYM_PER_WG
#define GR4PM_SYM_PER_WG 256
#endif
constexpr unsigned kSymPerWg = GR4PM_SYM_PER_WG; // output symbols (= threads) per workgroup
// One workgroup = up to kSymPerWg consecutive output symbols of ONE run.  The inputs of those symbols
// are one contiguous span (255*sps + arm_size items): it is staged into LDS with coalesced
// loads and every thread then reads its arm_size items from LDS (the MAC order of the
// reference, std::inner_product, m ascending, is kept: bit-exact).
// Everything a workgroup needs is resolved once by k_symf_wg_plan (a binary search inside the
// filter kernel would put ~12 dependent L2 round trips in front of each workgroup).
struct SymWg {
    long long lo_item; // oldest input item of the span (negative: inside the carried history)
    unsigned o0;       // first output symbol
    unsigned count;    // symbols (<= 256)
    unsigned arm;
    float scale;
    unsigned seg;      // fused CFC: segment of max(lo_item, 0)
    unsigned chan;     // index into the SymChan table (launches that span channels)
    // what the fused CFC needs of segment `seg` (RotSeg start / len / ck0, the increment and the counter that
    // k_rot_checkpoints left for it): one scalar load of this entry instead of three dependent ones in front of every
    // workgroup's first vector load.  Spans that run into further segments read those from the tables.
    unsigned long long seg_start, seg_len;
    unsigned seg_ck0, seg_counter0;
    cf seg_incr;
};
static_assert(sizeof(SymWg) == 64, "one 64-byte scalar load per workgroup");
// Fused CoarseFrequencyCorrection: when the symbol filter is fed by a CFC block, the rotation
// is applied while the filter stages its input (the rotated stream is never written to HBM).
struct CfcDev {
    const RotSeg* segs;   // this call's segments of channel 0, sorted by start, tiling [0, n_in)
    const cf* ck;         // phasor checkpoints every kRotChunk items
    const cf* seg_incr;
    const unsigned* seg_counter0;
    unsigned n_segs;
};
// One launch for every channel of a batch (gr4pm_cfc_symbol_filter_run_channels): what the single-channel launch
// passes as kernel arguments comes from a table, indexed by the channel of the workgroup's run.
struct SymChan {
    const cf* in;
    const cf* carry; // history of the channel's SymbolFilter (rotated items)
    cf* carry_next;
    cf* out;
    const RotSeg* segs; // the channel's share of the CFC plan
    const cf* seg_incr;
    const unsigned* seg_counter0;
    unsigned n_segs;
    unsigned pad;
    unsigned long long n; // items consumed by the channel in this call (history update)
    // two-piece input: items [0, n_head) of the call live at head[], item i >= n_head at in[i - n_head] (the
    // detector's delayed stream read in place: the tail of the batch before + this batch's input)
    const cf* head;
    unsigned long long n_head;
};
__device__ __forceinline__ CfcDev chan_cfc(const SymChan& c, const cf* ck)
{
    CfcDev f;
    f.segs = c.segs;
    f.ck = ck;
    f.seg_incr = c.seg_incr;
    f.seg_counter0 = c.seg_counter0;
    f.n_segs = c.n_segs;
    return f;
}
__device__ __forceinline__ unsigned cfc_find_seg(const CfcDev& f, long long idx)
{
    unsigned lo = 0, hi = f.n_segs - 1;
    const unsigned long long u = idx < 0 ? 0ull : static_cast<unsigned long long>(idx);
    while (lo < hi) {
        const unsigned mid = (lo + hi + 1) >> 1;
        if (f.segs[mid].start <= u) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
// rotated item idx (>= 0) of the current call: the lane replays at most kRotChunk-1 steps of
// the recurrence from its chunk's checkpoint
__device__ __forceinline__ cf cfc_phasor(const CfcDev& f, long long idx, unsigned seg)
{
    const unsigned long long j = static_cast<unsigned long long>(idx) - f.segs[seg].start;
    const unsigned long long c = j / kRotChunk;
    cf e = f.ck[f.segs[seg].ck0 + c];
    const cf inc = f.seg_incr[seg];
    unsigned counter = f.seg_counter0[seg] + static_cast<unsigned>(c * kRotChunk);
    const unsigned steps = static_cast<unsigned>(j - c * kRotChunk);
    for (unsigned t = 0; t < steps; ++t) rot_step(e, inc, counter);
    return e;
}
__device__ __forceinline__ cf cfc_item(const CfcDev& f, const cf* in, long long idx, unsigned seg)
{
    return cmul(in[idx], cfc_phasor(f, idx, seg)); // coarse_frequency_correction.hpp:87
}
// history after a fused call: last cap ROTATED items
__global__ void k_update_hist_cfc(const cf* __restrict__ in, const cf* __restrict__ carry, cf* __restrict__ carry_next,
                                  unsigned cap, size_t n, CfcDev f)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap) return;
    const long long idx = static_cast<long long>(n) - cap + i;
    carry_next[i] = idx < 0 ? carry[static_cast<long long>(cap) + idx] // history is stored rotated
                            : cfc_item(f, in, idx, cfc_find_seg(f, idx));
}

// the same for every channel of a batched launch (blockIdx.y = channel)
__global__ void k_update_hist_cfc_channels(const SymChan* __restrict__ chans, const cf* __restrict__ ck, unsigned cap)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap) return;
    const SymChan c = chans[blockIdx.y];
    if (c.n == 0) return;
    const long long idx = static_cast<long long>(c.n) - cap + i;
    const CfcDev f = chan_cfc(c, ck);
    if (idx < 0) {
        c.carry_next[i] = c.carry[static_cast<long long>(cap) + idx];
        return;
    }
    const cf x = static_cast<unsigned long long>(idx) < c.n_head ? c.head[idx] : c.in[idx - static_cast<long long>(c.n_head)];
    c.carry_next[i] = cmul(x, cfc_phasor(f, idx, cfc_find_seg(f, idx)));
}

__global__ void k_symf_wg_plan(const SymRun* __restrict__ runs, unsigned n_runs, unsigned n_wg, unsigned sps,
                               unsigned arm_size, CfcDev cfc, SymWg* __restrict__ plan,
                               const SymChan* __restrict__ chans, unsigned sym_per_wg)
{
    const unsigned w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_wg) return;
    unsigned lo = 0, hi = n_runs - 1;
    while (lo < hi) {
        const unsigned mid = (lo + hi + 1) >> 1;
        if (runs[mid].wg0 <= w) lo = mid;
        else hi = mid - 1;
    }
    const SymRun r = runs[lo];
    const unsigned first = (w - r.wg0) * sym_per_wg;
    SymWg p;
    p.o0 = r.out0 + first;
    p.count = min(sym_per_wg, r.count - first);
    p.lo_item = r.in0 + static_cast<long long>(first) * sps - (arm_size - 1);
    p.arm = r.arm;
    p.scale = r.scale;
    if (chans) cfc = chan_cfc(chans[r.chan], cfc.ck);
    p.seg = cfc.n_segs ? cfc_find_seg(cfc, p.lo_item) : 0u;
    p.chan = r.chan;
    p.seg_start = p.seg_len = 0;
    p.seg_ck0 = p.seg_counter0 = 0;
    p.seg_incr = cf{ 0.f, 0.f };
    if (cfc.n_segs) {
        const RotSeg g = cfc.segs[p.seg];
        p.seg_start = g.start, p.seg_len = g.len, p.seg_ck0 = g.ck0;
        p.seg_incr = cfc.seg_incr[p.seg];
        p.seg_counter0 = cfc.seg_counter0[p.seg];
    }
    plan[w] = p;
}

// Fused CFC: fills the workgroup's tile (phase-major: item i at (i % sps) * pitch + i / sps) with the ROTATED items of
// the span [p.lo_item, p.lo_item + span).
//  1. history items are stored rotated: straight to the tile
//  2. one lane per checkpoint chunk: the lane reads its kRotChunk raw items (64 contiguous bytes) straight from global
//     memory, replays the phasor recurrence of the chunk once (kRotChunk-1 steps for kRotChunk items) and writes the
//     rotated items to the tile; segment by segment (usually one).  The raw items are not staged in LDS (round 1 did):
//     half the LDS footprint, one barrier and one global-memory latency less per workgroup.
// ORIGIN (a multiple of sps and of kRotChunk): item i of the span lives at tile index i + ORIGIN, and a chunk that
// only PARTLY overlaps the span is written whole, its other items into the ORIGIN entries in front of the span or the
// kRotChunk behind it -- as long as the whole chunk lies inside its segment (then its raw items exist).  With
// ORIGIN = 0 a partly overlapping chunk goes item by item through the path at the bottom (about 220 instructions for
// its whole wave): the first and the last chunk of almost every span, i.e. both waves of every workgroup of the
// receiver's filter.
template <unsigned THREADS, unsigned ORIGIN = 0>
__device__ __forceinline__ void cfc_fill_tile(const SymWg& p, unsigned span, unsigned sps, unsigned pitch, cf* tile,
                                              const cf* __restrict__ in, const cf* __restrict__ carry, unsigned cap,
                                              const CfcDev& cfc, const cf* __restrict__ head = nullptr,
                                              long long n_head = 0)
{
    if (p.lo_item < 0)
        for (unsigned i = threadIdx.x; i < span && p.lo_item + i < 0; i += THREADS)
            tile[((i + ORIGIN) % sps) * pitch + (i + ORIGIN) / sps] = carry[static_cast<long long>(cap) + p.lo_item + i];
    const long long lo = p.lo_item < 0 ? 0 : p.lo_item;
    const long long hi = p.lo_item + span;
    for (unsigned sg = p.seg; sg < cfc.n_segs; ++sg) {
        RotSeg g;
        cf inc;
        unsigned c0;
        if (sg == p.seg) { // (uniform) the usual case, and the only segment of most spans: everything is in the plan entry
            g.start = p.seg_start, g.len = p.seg_len, g.ck0 = p.seg_ck0;
            inc = p.seg_incr, c0 = p.seg_counter0;
        } else {
            g = cfc.segs[sg];
            inc = cfc.seg_incr[sg], c0 = cfc.seg_counter0[sg];
        }
        const long long a = max(static_cast<long long>(g.start), lo);
        const long long b = min(static_cast<long long>(g.start + g.len), hi);
        if (a < b) {
            const unsigned long long c_first = static_cast<unsigned long long>(a - g.start) / kRotChunk;
            const unsigned n_chunks =
                static_cast<unsigned>(static_cast<unsigned long long>(b - 1 - g.start) / kRotChunk - c_first) + 1;
            for (unsigned ch = threadIdx.x; ch < n_chunks; ch += THREADS) {
                const unsigned long long c = c_first + ch;
                cf e = cfc.ck[g.ck0 + c];
                unsigned counter = c0 + static_cast<unsigned>(c * kRotChunk);
                const long long idx0 = static_cast<long long>(g.start + c * kRotChunk);
                const bool whole = ORIGIN ? idx0 + static_cast<long long>(kRotChunk) <= static_cast<long long>(g.start + g.len)
                                          : idx0 >= a && idx0 + static_cast<long long>(kRotChunk) <= b;
                if (whole && (counter & 511u) <= 512u - kRotChunk &&
                    (idx0 >= n_head || idx0 + static_cast<long long>(kRotChunk) <= n_head)) {
                    // whole chunk inside the span or (ORIGIN) at least inside the segment, on one side of a two-piece
                    // input, and no renormalisation among its 7 steps (the usual case): straight-line packed arithmetic,
                    // same operations as below.  (With ORIGIN the index can start up to kRotChunk - 1 in front of the span.)
                    const unsigned i0 = static_cast<unsigned>(idx0 - p.lo_item + static_cast<long long>(ORIGIN));
                    // (explicitly a global-memory pointer: in the multi-channel launch `in` / `head` are loaded from the
                    // channel table, which makes them generic pointers and these loads flat_load -- both address paths,
                    // both wait counters -- instead of global_load)
                    typedef const float __attribute__((address_space(1))) * gflt;
                    const gflt src = (gflt)(idx0 >= n_head ? in + (idx0 - n_head) : head + idx0);
                    cf x[kRotChunk];
#pragma unroll
                    for (unsigned t = 0; t < kRotChunk; ++t) x[t] = cf{ src[2 * t], src[2 * t + 1] };
                    rot8_pk(x, e, inc); // hpp:87
                    if (sps == 4) { // items t and t + 4 share their phase row and sit side by side: four addresses, not eight
#pragma unroll
                        for (unsigned t = 0; t < 4; ++t) {
                            const unsigned i = i0 + t;
                            cf* q = tile + (i % 4) * pitch + i / 4;
                            q[0] = x[t];
                            q[1] = x[t + 4];
                        }
                    } else {
#pragma unroll
                        for (unsigned t = 0; t < kRotChunk; ++t) {
                            const unsigned i = i0 + t;
                            tile[(i % sps) * pitch + i / sps] = x[t];
                        }
                    }
                    continue;
                }
#pragma unroll
                for (unsigned t = 0; t < kRotChunk; ++t) {
                    const long long idx = idx0 + t;
                    if (idx >= a && idx < b) {
                        const unsigned i = static_cast<unsigned>(idx - p.lo_item) + ORIGIN;
                        const cf x = idx < n_head ? head[idx] : in[idx - n_head];
                        tile[(i % sps) * pitch + i / sps] = cmul(x, e); // hpp:87
                    }
                    if (t + 1 < kRotChunk) rot_step(e, inc, counter);
                }
            }
        }
        if (static_cast<long long>(g.start + g.len) >= hi) break;
    }
}

// SPS > 0: samples_per_symbol known at compile time (divisions become shifts / constants);
// SPS == 0: run-time value.
template <typename T, int SPS, bool CFC>
__global__ __launch_bounds__(kSymPerWg) void k_symbol_filter(const T* __restrict__ in, const T* __restrict__ carry,
                                                       unsigned cap, const float* __restrict__ taps,
                                                       unsigned arm_size, unsigned sps_rt,
                                                       const SymWg* __restrict__ plan, T* __restrict__ out,
                                                       CfcDev cfc, const SymChan* __restrict__ chans)
{
    extern __shared__ unsigned char s_raw[];
    T* tile = reinterpret_cast<T*>(s_raw);
    const unsigned sps = SPS > 0 ? static_cast<unsigned>(SPS) : sps_rt;
    const SymWg p = plan[blockIdx.x];
    const cf* head = nullptr;
    long long n_head = 0;
    if constexpr (CFC) {
        if (chans) { // a launch that spans channels: the workgroup's channel supplies the pointers
            const SymChan c = chans[p.chan];
            in = c.in;
            carry = c.carry;
            out = c.out;
            cfc = chan_cfc(c, cfc.ck);
            head = c.head;
            n_head = static_cast<long long>(c.n_head);
        }
    }
    const unsigned span = (p.count - 1) * sps + arm_size;
    // tile is stored phase-major: item i lives at (i % sps) * pitch + i / sps, so that for a
    // fixed tap m the 64 lanes (items sps apart) read consecutive LDS words
    const unsigned pitch = (kSymPerWg * sps + arm_size) / sps + 2;
    // the arm is the same for the whole workgroup: its taps go to LDS (broadcast reads)
    float* s_arm = reinterpret_cast<float*>(tile + pitch * sps);
    for (unsigned m = threadIdx.x; m < arm_size; m += kSymPerWg) s_arm[m] = taps[static_cast<size_t>(p.arm) * arm_size + m];
    if constexpr (CFC) {
        cfc_fill_tile<kSymPerWg>(p, span, sps, pitch, tile, in, carry, cap, cfc, head, n_head);
    } else {
        for (unsigned i = threadIdx.x; i < span; i += kSymPerWg)
            tile[(i % sps) * pitch + i / sps] = item_at(in, carry, cap, p.lo_item + i);
    }
    __syncthreads();
    if (threadIdx.x < p.count) {
        // tile index of tap m of this symbol: tid * sps + j with j = arm_size - 1 - m;
        // j % sps and j / sps are the same for every thread
        T acc = zero_item(T{});
        for (unsigned m = 0; m < arm_size; ++m) {
            const unsigned j = arm_size - 1 - m;
            acc = mac(acc, s_arm[m], tile[(j % sps) * pitch + j / sps + threadIdx.x]);
        }
        out[p.o0 + threadIdx.x] = scale_item(p.scale, acc);
    }
}

// The receiver's design (4 samples per symbol, 44-tap arms, fused CFC) as its own kernel.  Measured on the kernel above
// (343 us per 2^26 samples): no MACs -76 us, no rotation -31, no item loads -63, empty workgroups 26 -- VALU (~0.10 ms),
// the LDS pipe (~0.15 ms: 44 8-byte tile reads and 44 tap reads per symbol) and HBM (0.13 ms) add up instead of
// overlapping.  Here the LDS traffic of the MACs is 45 % of that:
//   * a lane computes TWO neighbouring symbols; they share 40 of their 44 items, and one 16-byte read delivers the two
//     tile entries (phase row, items 2l + 2k and 2l + 2k + 1) that the pair needs at one tap position: 24 ds_read_b128
//     per two symbols instead of 88 ds_read_b64
//   * the 44 taps of the workgroup's arm are uniform: scalar loads into SGPRs, no LDS copy, no tap reads
//   * 240 symbols per workgroup of 128 threads: the span is 1000 items = at most 126 checkpoint chunks, one pass of the
//     rotation phase with 98 % of the lanes busy (256 symbols: 134 chunks on 256 lanes)
// MAC order as in the reference (std::inner_product, tap index ascending), every product and sum rounded once: bit-exact.
constexpr unsigned kFastSym = 240, kFastThreads = 128, kFastArm = 44, kFastSps = 4;
constexpr unsigned kFastOrigin = 8; // tile index of the span's first item: room for a chunk that starts in front of it
constexpr unsigned kFastPitch = 256; // entries per phase row: (8 + 1000 + 7) / 4 = 254 used, 8 KiB per tile
static_assert(kFastPitch % 2 == 0 && kFastPitch * kFastSps >= kFastOrigin + (kFastSym - 1) * kFastSps + kFastArm + kRotChunk - 1 &&
                  kFastOrigin % 8 == 0,
              "16-byte reads need even rows; the margins of partly overlapping chunks need room");
// ABL (timing only, wrong results; GR4PM_SYMF_ABL): 1 = no MAC phase, 2 = no tile fill (no item loads, no rotation)
// (second launch bound: eight waves per SIMD, i.e. at most 64 VGPRs -- hipcc takes 80 when left alone, and the kernel is
// bound by the workgroups a CU holds: 16 instead of 12)
// Everything uniform stays on the scalar unit (round 5: 218.5 M -> 166.5 M vector wave-instructions per 2^28 samples, 391 ->
// 298 per wave and tile of which 176 are the multiply-adds; 558 -> 521 us alone = 5.2 TB/s of input + output):
//   * the channel's pointers come from ONE table entry through scalar loads -- the single-channel launch passes its entry
//     by value as the FIRST kernel argument and the kernel reads it where it lies in the kernarg segment, so both launch
//     forms share one code path and nothing of it stays live across the multiply-adds (the 44 taps need 44 SGPRs there;
//     with separate in / carry / out / CfcDev arguments hipcc spilled ~65 SGPRs per tile through v_writelane / v_readlane)
//   * further segments of a span are read through constant-address-space pointers (s_load; hipcc reads them with
//     flat_load when it cannot prove the tables unwritten, which made every index of the fill a 64-bit vector value)
//   * per lane only ch * 8 varies: chunk c_first + ch of the segment; checkpoint, items and tile slots are a uniform
//     base plus that, the four tile addresses of a chunk are (uniform phase row and column of item t) + 16 ch bytes
// Bit-exact as before: same packed products and sums (rot8_pk), same item-by-item path for the chunks that overlap a
// segment end, the head / input seam of a two-piece input, or a renormalisation.
typedef const unsigned long long __attribute__((address_space(4)))* symf_cu64;
typedef const unsigned __attribute__((address_space(4)))* symf_cu32;
typedef const float __attribute__((address_space(4)))* symf_cf32;
static_assert(sizeof(SymChan) == 88 && offsetof(SymChan, segs) == 32 && offsetof(SymChan, n_segs) == 56 &&
                  offsetof(SymChan, head) == 72 && offsetof(SymChan, n_head) == 80 && sizeof(RotSeg) == 48 &&
                  offsetof(RotSeg, ck0) == 20,
              "k_symbol_filter_fast reads these tables word by word");
template <int ABL, bool LOOP>
__global__ __launch_bounds__(kFastThreads, 8) void k_symbol_filter_fast(SymChan one, const SymChan* __restrict__ chans,
                                                                     const SymWg* __restrict__ plan,
                                                                     const float* __restrict__ taps,
                                                                     const cf* __restrict__ ck, unsigned cap, unsigned n_wg,
                                                                     unsigned tiles)
{
    (void)one; // read in place: the first 88 bytes of the kernarg segment
    __shared__ __attribute__((aligned(16))) cf tile[kFastSps * kFastPitch];
    // LOOP (GR4PM_SYMF_TILES > 1; the default is one tile per workgroup since round 5): `tiles` consecutive plan entries
    // per workgroup, the entry of the NEXT tile requested (one 64-byte scalar load) while this tile's results are stored.
    // Round 3 ran two tiles per workgroup with the next entry requested in FRONT of the tile's work; its 16 SGPRs do
    // not fit beside the 44 taps (80 SGPRs at eight waves per SIMD) and the loop-carried state cost ~50 v_writelane /
    // v_readlane per tile.  Measured with this kernel: 521 us with one tile, 538 with two (184.3 M instructions).
    unsigned w = blockIdx.x * tiles;
    const unsigned w_end = LOOP ? min(w + tiles, n_wg) : w + 1; // (!LOOP: one tile, tiles == 1)
    SymWg p = plan[w];
    for (; w < w_end; ++w) {
    const unsigned span = (p.count - 1) * kFastSps + kFastArm;
    cf* out;
    {
    const symf_cu64 cw = chans ? (symf_cu64)(chans + p.chan) : (symf_cu64)__builtin_amdgcn_kernarg_segment_ptr();
    out = reinterpret_cast<cf*>(cw[3]);
    if (!(ABL & 2)) {
    const cf* in = reinterpret_cast<const cf*>(cw[0]);
    const cf* head = reinterpret_cast<const cf*>(cw[9]);
    const long long n_head = static_cast<long long>(cw[10]);
    const unsigned n_segs = static_cast<unsigned>(cw[7]);
    if (p.lo_item < 0) { // the carried history is stored rotated: straight to the tile
        const cf* carry = reinterpret_cast<const cf*>(cw[1]);
        for (unsigned i = threadIdx.x; i < span && p.lo_item + i < 0; i += kFastThreads)
            tile[((i + kFastOrigin) % kFastSps) * kFastPitch + (i + kFastOrigin) / kFastSps] =
                carry[static_cast<long long>(cap) + p.lo_item + i];
    }
    const long long lo = p.lo_item < 0 ? 0 : p.lo_item;
    const long long hi = p.lo_item + span;
    for (unsigned sg = p.seg; sg < n_segs; ++sg) {
        unsigned long long g_start, g_len;
        unsigned g_ck0, c0;
        cf inc;
        if (sg == p.seg) { // the usual case, and the only segment of most spans: everything is in the plan entry
            g_start = p.seg_start, g_len = p.seg_len, g_ck0 = p.seg_ck0;
            inc = p.seg_incr, c0 = p.seg_counter0;
        } else {
            const symf_cu64 gw = (symf_cu64)(reinterpret_cast<const RotSeg*>(cw[4]) + sg);
            g_start = gw[0], g_len = gw[1];
            g_ck0 = ((symf_cu32)gw)[5];
            const symf_cf32 iw = (symf_cf32)(reinterpret_cast<const cf*>(cw[5]) + sg);
            inc = cf{ iw[0], iw[1] };
            c0 = ((symf_cu32)cw[6])[sg];
        }
        const long long g_end = static_cast<long long>(g_start + g_len);
        const long long a = max(static_cast<long long>(g_start), lo);
        const long long b = min(g_end, hi);
        if (a < b) {
            const unsigned long long c_first = static_cast<unsigned long long>(a - g_start) / kRotChunk;
            const unsigned n_chunks =
                static_cast<unsigned>(static_cast<unsigned long long>(b - 1 - g_start) / kRotChunk - c_first) + 1;
            // (uniform) chunk ch of this pass: items first + 8 ch ..., checkpoint ck_s[ch], counter counter_s + 8 ch,
            // tile slots from i0_s + 8 ch on
            const long long first = static_cast<long long>(g_start + c_first * kRotChunk);
            const cf* ck_s = ck + (g_ck0 + c_first);
            const unsigned counter_s = c0 + static_cast<unsigned>(c_first * kRotChunk);
            const unsigned i0_s = static_cast<unsigned>(first - p.lo_item + static_cast<long long>(kFastOrigin));
            // items of the segment from `first` on (whole chunks only on the straight path)
            const unsigned room = static_cast<unsigned>(min(g_end - first, static_cast<long long>(0x7fffffff)));
            // every chunk of the pass on one side of a two-piece input's seam?  (else: item by item)
            const bool in_side = first >= n_head;
            const bool one_side = in_side || first + static_cast<long long>(n_chunks * kRotChunk) <= n_head;
            typedef const float __attribute__((address_space(1))) * gflt;
            const gflt src_s = (gflt)(in_side ? in + (first - n_head) : head + first);
            for (unsigned ch = threadIdx.x; ch < n_chunks; ch += kFastThreads) {
                const unsigned t8 = ch * kRotChunk;
                cf e = ck_s[ch];
                unsigned counter = counter_s + t8;
                if (one_side && t8 + kRotChunk <= room && (counter & 511u) <= 512u - kRotChunk) {
                    const gflt src = src_s + 2 * t8;
                    cf x[kRotChunk];
#pragma unroll
                    for (unsigned t = 0; t < kRotChunk; ++t) x[t] = cf{ src[2 * t], src[2 * t + 1] };
                    rot8_pk(x, e, inc); // hpp:87
                    // items t and t + 4 share their phase row and sit side by side: four addresses, not eight
#pragma unroll
                    for (unsigned t = 0; t < 4; ++t) {
                        const unsigned it = i0_s + t; // (uniform)
                        cf* q = tile + ((it % kFastSps) * kFastPitch + it / kFastSps) + 2 * ch;
                        q[0] = x[t];
                        q[1] = x[t + 4];
                    }
                    continue;
                }
                const long long idx0 = first + t8;
#pragma unroll
                for (unsigned t = 0; t < kRotChunk; ++t) {
                    const long long idx = idx0 + t;
                    if (idx >= a && idx < b) {
                        const unsigned i = static_cast<unsigned>(idx - p.lo_item) + kFastOrigin;
                        const cf x = idx < n_head ? head[idx] : in[idx - n_head];
                        tile[(i % kFastSps) * kFastPitch + i / kFastSps] = cmul(x, e); // hpp:87
                    }
                    if (t + 1 < kRotChunk) rot_step(e, inc, counter);
                }
            }
        }
        if (g_end >= hi) break;
    }
    }
    }
    const float* __restrict__ tp = taps + static_cast<size_t>(p.arm) * kFastArm; // uniform: scalar loads
    float tap[kFastArm];
#pragma unroll
    for (unsigned m = 0; m < kFastArm; ++m) tap[m] = tp[m];
    __syncthreads();
    const unsigned l = threadIdx.x;
    if (2 * l < p.count) {
    if (ABL & 1) {
        out[p.o0 + 2 * l] = cf{ tap[0], tap[1] };
        if (2 * l + 1 < p.count) out[p.o0 + 2 * l + 1] = cf{ tap[2], tap[3] };
    } else {
    // pair(ph, k) = tile entries (ph, 2l + 2k) and (ph, 2l + 2k + 1); symbol A = 2l uses entry 2l + q at tap position
    // q = j / 4 of phase ph = j % 4 (j = 43 - m), symbol B = 2l + 1 uses entry 2l + 1 + q
    const float4* rows = reinterpret_cast<const float4*>(tile) + l + kFastOrigin / (2 * kFastSps); // two entries per float4
    constexpr unsigned kRow4 = kFastPitch / 2; // float4 per phase row
    // The MACs as packed FP32: v_pk_mul_f32 (re, im) x (tap, tap) -- the tap broadcast from one half of an SGPR pair by
    // op_sel -- and v_pk_add_f32 onto the accumulator: every product and every sum still rounded once, in the
    // reference's order, in 2 instead of 4 instructions per tap and symbol.  One statement per tap position (four
    // phases, both symbols: 16 instructions; hipcc pads register overlaps BETWEEN asm statements with s_nop).
    typedef float f2 __attribute__((ext_vector_type(2)));
    f2 accA = { 0.f, 0.f }, accB = { 0.f, 0.f };
    // a3 .. a0 / b3 .. b0: the entries of phases 3 .. 0 for symbol A / B at this tap position; t01, t23: the four taps
    // (ascending index) that go with phases 3, 2, 1, 0
    auto mac4 = [&](f2 a3, f2 b3, f2 a2, f2 b2, f2 a1, f2 b1, f2 a0, f2 b0, f2 t01, f2 t23) {
        f2 pa, pb;
        asm("v_pk_mul_f32 %2, %4, %12 op_sel_hi:[1,0]\n\t"
            "v_pk_mul_f32 %3, %5, %12 op_sel_hi:[1,0]\n\t"
            "v_pk_add_f32 %0, %0, %2\n\t"
            "v_pk_add_f32 %1, %1, %3\n\t"
            "v_pk_mul_f32 %2, %6, %12 op_sel:[0,1]\n\t"
            "v_pk_mul_f32 %3, %7, %12 op_sel:[0,1]\n\t"
            "v_pk_add_f32 %0, %0, %2\n\t"
            "v_pk_add_f32 %1, %1, %3\n\t"
            "v_pk_mul_f32 %2, %8, %13 op_sel_hi:[1,0]\n\t"
            "v_pk_mul_f32 %3, %9, %13 op_sel_hi:[1,0]\n\t"
            "v_pk_add_f32 %0, %0, %2\n\t"
            "v_pk_add_f32 %1, %1, %3\n\t"
            "v_pk_mul_f32 %2, %10, %13 op_sel:[0,1]\n\t"
            "v_pk_mul_f32 %3, %11, %13 op_sel:[0,1]\n\t"
            "v_pk_add_f32 %0, %0, %2\n\t"
            "v_pk_add_f32 %1, %1, %3"
            : "+v"(accA), "+v"(accB), "=&v"(pa), "=&v"(pb)
            : "v"(a3), "v"(b3), "v"(a2), "v"(b2), "v"(a1), "v"(b1), "v"(a0), "v"(b0), "s"(t01), "s"(t23));
    };
    auto lo2 = [](const float4& v) { return f2{ v.x, v.y }; };
    auto hi2 = [](const float4& v) { return f2{ v.z, v.w }; };
    float4 hi[kFastSps], lo[kFastSps];
#pragma unroll
    for (unsigned ph = 0; ph < kFastSps; ++ph) hi[ph] = rows[ph * kRow4 + 5];
#pragma unroll
    for (int k = 5; k >= 0; --k) {
        if (k > 0) {
#pragma unroll
            for (unsigned ph = 0; ph < kFastSps; ++ph) lo[ph] = rows[ph * kRow4 + (k - 1)];
        }
        asm volatile("" ::: "memory"); // the reads of the next pair stay here, ahead of the MACs that hide them
        {   // q = 2k: A <- pair.lo, B <- pair.hi; taps 40 - 8k .. 43 - 8k
            const int m0 = static_cast<int>(kFastArm) - 4 - 4 * (2 * k);
            mac4(lo2(hi[3]), hi2(hi[3]), lo2(hi[2]), hi2(hi[2]), lo2(hi[1]), hi2(hi[1]), lo2(hi[0]), hi2(hi[0]),
                 f2{ tap[m0], tap[m0 + 1] }, f2{ tap[m0 + 2], tap[m0 + 3] });
        }
        if (k > 0) { // q = 2k - 1: A <- pair(k - 1).hi, B <- pair(k).lo
            const int m0 = static_cast<int>(kFastArm) - 4 - 4 * (2 * k - 1);
            mac4(hi2(lo[3]), lo2(hi[3]), hi2(lo[2]), lo2(hi[2]), hi2(lo[1]), lo2(hi[1]), hi2(lo[0]), lo2(hi[0]),
                 f2{ tap[m0], tap[m0 + 1] }, f2{ tap[m0 + 2], tap[m0 + 3] });
#pragma unroll
            for (unsigned ph = 0; ph < kFastSps; ++ph) hi[ph] = lo[ph];
        }
    }
    out[p.o0 + 2 * l] = scale_item(p.scale, cf{ accA.x, accA.y });
    if (2 * l + 1 < p.count) out[p.o0 + 2 * l + 1] = scale_item(p.scale, cf{ accB.x, accB.y });
    }
    }
    if (w + 1 < w_end) {
        p = plan[w + 1]; // (requested here, behind the multiply-adds: in front of them its 16 SGPRs do not fit beside the taps)
        __syncthreads(); // the tile is free for the next fill
    }
    }
}

// Long arms (BASELINE configs[4]: 32 arms x 1025 taps, 4 samples per symbol), plain SymbolFilter on complex items: the
// generic kernel above reads one 8-byte item and one tap from LDS per multiply-add (12 bytes per tap and symbol: 15 Gsps
// in, bound by the LDS pipe).  Here, as in k_symbol_filter_fast: a lane computes TWO neighbouring symbols, one
// ds_read_b128 delivers the two tile entries the pair needs at one tap position of one phase (4 bytes per tap and
// symbol), the arm's taps are uniform and stream through SGPRs (scalar loads, eight a time, the next eight requested
// before the current ones are used), and the multiply-adds are v_pk_mul_f32 / v_pk_add_f32 with the tap broadcast from
// an SGPR pair -- every product and every sum rounded once, tap index ascending (symbol_filter.hpp:208-214): bit-exact.
// Tap m of symbol s sits on tile item 4 s + j, j = arm_size - 1 - m: phase j % 4, entry s + j / 4 of the phase row.
// The arm starts with (arm_size - 1) % 4 + 1 "head" taps on the top tap position, then whole tap positions of four.
__global__ __launch_bounds__(kFastThreads, 8) void k_symbol_filter_long(const cf* __restrict__ in, const cf* __restrict__ carry,
                                                                      unsigned cap, const float* __restrict__ taps,
                                                                      unsigned arm_size, unsigned pitch,
                                                                      const SymWg* __restrict__ plan, cf* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_long_raw[];
    cf* tile = reinterpret_cast<cf*>(s_long_raw);
    const SymWg p = plan[blockIdx.x];
    const unsigned span = (p.count - 1) * kFastSps + arm_size;
    for (unsigned i = threadIdx.x; i < span; i += kFastThreads)
        tile[(i % kFastSps) * pitch + i / kFastSps] = item_at(in, carry, cap, p.lo_item + i);
    __syncthreads();
    const unsigned l = threadIdx.x;
    if (2 * l >= p.count) return;
    typedef float f2 __attribute__((ext_vector_type(2)));
    const float* __restrict__ tp = taps + static_cast<size_t>(p.arm) * arm_size; // uniform: scalar loads
    f2 accA = { 0.f, 0.f }, accB = { 0.f, 0.f };
    const unsigned J = arm_size - 1, q_top = J / kFastSps, r = J % kFastSps;
    // head taps m = 0 .. r: phases r .. 0 of tap position q_top
    for (unsigned m = 0; m <= r; ++m) {
        const unsigned ph = r - m;
        const cf a = tile[ph * pitch + 2 * l + q_top], b = tile[ph * pitch + 2 * l + 1 + q_top];
        const float t = tp[m];
        accA = f2{ accA.x + t * a.x, accA.y + t * a.y };
        accB = f2{ accB.x + t * b.x, accB.y + t * b.y };
    }
    // a3 .. a0 / b3 .. b0: the entries of phases 3 .. 0 for symbol A / B at one tap position; t01, t23: its four taps
    auto mac4 = [&](f2 a3, f2 b3, f2 a2, f2 b2, f2 a1, f2 b1, f2 a0, f2 b0, f2 t01, f2 t23) {
        f2 pa, pb;
        asm("v_pk_mul_f32 %2, %4, %12 op_sel_hi:[1,0]\n\t"
            "v_pk_mul_f32 %3, %5, %12 op_sel_hi:[1,0]\n\t"
            "v_pk_add_f32 %0, %0, %2\n\t"
            "v_pk_add_f32 %1, %1, %3\n\t"
            "v_pk_mul_f32 %2, %6, %12 op_sel:[0,1]\n\t"
            "v_pk_mul_f32 %3, %7, %12 op_sel:[0,1]\n\t"
            "v_pk_add_f32 %0, %0, %2\n\t"
            "v_pk_add_f32 %1, %1, %3\n\t"
            "v_pk_mul_f32 %2, %8, %13 op_sel_hi:[1,0]\n\t"
            "v_pk_mul_f32 %3, %9, %13 op_sel_hi:[1,0]\n\t"
            "v_pk_add_f32 %0, %0, %2\n\t"
            "v_pk_add_f32 %1, %1, %3\n\t"
            "v_pk_mul_f32 %2, %10, %13 op_sel:[0,1]\n\t"
            "v_pk_mul_f32 %3, %11, %13 op_sel:[0,1]\n\t"
            "v_pk_add_f32 %0, %0, %2\n\t"
            "v_pk_add_f32 %1, %1, %3"
            : "+v"(accA), "+v"(accB), "=&v"(pa), "=&v"(pb)
            : "v"(a3), "v"(b3), "v"(a2), "v"(b2), "v"(a1), "v"(b1), "v"(a0), "v"(b0), "s"(t01), "s"(t23));
    };
    auto lo2 = [](const float4& v) { return f2{ v.x, v.y }; };
    auto hi2 = [](const float4& v) { return f2{ v.z, v.w }; };
    // pair(ph, k) = tile entries (ph, 2l + 2k) and (ph, 2l + 2k + 1): symbol A uses entry 2l + q at tap position q,
    // symbol B entry 2l + 1 + q, so q = 2k takes (pair k .lo, pair k .hi) and q = 2k + 1 takes (pair k .hi, pair k+1 .lo)
    const float4* rows = reinterpret_cast<const float4*>(tile) + l;
    const unsigned row4 = pitch / 2; // float4 per phase row
    auto load_pair = [&](float4(&v)[kFastSps], unsigned k) {
#pragma unroll
        for (unsigned ph = 0; ph < kFastSps; ++ph) v[ph] = rows[ph * row4 + k];
    };
    auto even = [&](const float4(&P)[kFastSps], const float* t) { // q = 2k
        mac4(lo2(P[3]), hi2(P[3]), lo2(P[2]), hi2(P[2]), lo2(P[1]), hi2(P[1]), lo2(P[0]), hi2(P[0]), f2{ t[0], t[1] }, f2{ t[2], t[3] });
    };
    auto odd = [&](const float4(&P)[kFastSps], const float4(&Pn)[kFastSps], const float* t) { // q = 2k + 1, Pn = pair k + 1
        mac4(hi2(P[3]), lo2(Pn[3]), hi2(P[2]), lo2(Pn[2]), hi2(P[1]), lo2(Pn[1]), hi2(P[0]), lo2(Pn[0]), f2{ t[0], t[1] }, f2{ t[2], t[3] });
    };
    if (q_top > 0) {
        // eight taps with ONE scalar load (s_load_dwordx8; the address only needs dword alignment)
        typedef float f8 __attribute__((ext_vector_type(8), aligned(4)));
        unsigned m = r + 1;     // next tap
        unsigned Q = q_top - 1; // next tap position
        float4 P0[kFastSps], P1[kFastSps];
        unsigned k = Q / 2;
        load_pair(P0, k);
        if (Q & 1u) {
            load_pair(P1, k + 1);
            float t[4] = { tp[m], tp[m + 1], tp[m + 2], tp[m + 3] };
            odd(P0, P1, t);
            m += 4;
        }
        {
            float t[4] = { tp[m], tp[m + 1], tp[m + 2], tp[m + 3] };
            even(P0, t);
            m += 4;
        }
        // From here on two tap positions (eight taps) per pass, two passes per iteration with the pair registers P0 / P1
        // taking turns (no moves).  The pair of the NEXT pass is requested between the two halves of a pass -- its
        // registers are free once odd() has used their .lo halves -- so sixteen packed instructions cover the LDS
        // latency; the sixteen taps of the next iteration are requested before this iteration's are used.
        if (k > 0) load_pair(P1, k - 1);
        f8 ta = *reinterpret_cast<const f8*>(tp + m), tb = *reinterpret_cast<const f8*>(tp + min(m + 8, arm_size - 8));
        while (k >= 2) {
            const f8 ua = ta, ub = tb;
            m += 16;
            // (clamped: the last iterations request taps they do not use instead of branching)
            ta = *reinterpret_cast<const f8*>(tp + min(m, arm_size - 8));
            tb = *reinterpret_cast<const f8*>(tp + min(m + 8, arm_size - 8));
            {
                const float t[8] = { ua[0], ua[1], ua[2], ua[3], ua[4], ua[5], ua[6], ua[7] };
                odd(P1, P0, t); // pass a: pair k - 1, tap positions 2k - 1 and 2k - 2
                load_pair(P0, k - 2);
                asm volatile("" ::: "memory"); // the request stays here, in front of the sixteen instructions that hide it
                even(P1, t + 4);
            }
            {
                const float t[8] = { ub[0], ub[1], ub[2], ub[3], ub[4], ub[5], ub[6], ub[7] };
                odd(P0, P1, t); // pass b: pair k - 2
                if (k >= 3) load_pair(P1, k - 3);
                asm volatile("" ::: "memory");
                even(P0, t + 4);
            }
            k -= 2;
        }
        if (k == 1) {
            const float t[8] = { ta[0], ta[1], ta[2], ta[3], ta[4], ta[5], ta[6], ta[7] };
            odd(P1, P0, t);
            even(P1, t + 4);
        }
    }
    out[p.o0 + 2 * l] = scale_item(p.scale, cf{ accA.x, accA.y });
    if (2 * l + 1 < p.count) out[p.o0 + 2 * l + 1] = scale_item(p.scale, cf{ accB.x, accB.y });
}
// which (fused, item type, sps, arm size) combinations run it
// (its tile: entries per phase row = the last symbol's entry at the top tap position, + 1 for symbol B; even)
static unsigned symf_long_pitch(size_t arm_size) { return ((kFastSym + (static_cast<unsigned>(arm_size) - 1) / kFastSps + 2) + 1u) & ~1u; }
static size_t symf_long_lds(size_t arm_size) { return static_cast<size_t>(kFastSps) * symf_long_pitch(arm_size) * sizeof(cf); }
static bool symf_long(bool fused, bool cf_items, size_t sps, size_t arm_size)
{
    static const bool off = getenv("GR4PM_SYMF_GENERIC") != nullptr;
    // arms whose tile does not fit the LDS (arm sizes beyond ~20 000) stay with the generic kernel
    return !fused && cf_items && sps == kFastSps && arm_size >= 64 && symf_long_lds(arm_size) <= kFirMaxSmem && !off;
}

#ifdef GR4PM_EXPERIMENTS
// GR4PM_TIMING_SKIP=symf_fake / costas_fake: timing experiments only.  Stand-ins with the memory traffic (symbol
// filter) or the life time (Costas) of the kernel they replace and at most 32 VGPRs, no LDS: what would the chain
// gain if the real kernel fitted beside two 240-VGPR correlator waves of every SIMD?
__global__ __launch_bounds__(kFastThreads) void k_symf_fake(const cf* __restrict__ in, const SymWg* __restrict__ plan,
                                                           cf* __restrict__ out)
{
    const SymWg p = plan[blockIdx.x];
    const float4* ip = reinterpret_cast<const float4*>(in + (p.lo_item > 0 ? (p.lo_item & ~1ll) : 0));
    float4 a = ip[threadIdx.x], b = ip[threadIdx.x + 128], c = ip[threadIdx.x + 256];
    float4 d = threadIdx.x < 96 ? ip[threadIdx.x + 384] : a;
    a.x += b.x + c.x + d.x, a.y += b.y + c.y + d.y, a.z += b.z + c.z + d.z, a.w += b.w + c.w + d.w;
    if (threadIdx.x < 120) reinterpret_cast<float4*>(out + (p.o0 & ~1u))[threadIdx.x] = a;
}
#endif

// symbols per workgroup of the kernel that a (fused, sps, arm size) combination runs
static bool symf_fast(bool fused, size_t sps, size_t arm_size)
{
    static const bool off = getenv("GR4PM_SYMF_GENERIC") != nullptr; // A/B switch: the generic kernel for every design
    return fused && sps == kFastSps && arm_size == kFastArm && !off;
}
static unsigned symf_per_wg(bool fused, size_t sps, size_t arm_size, bool cf_items = true)
{
    return (symf_fast(fused, sps, arm_size) || symf_long(fused, cf_items, sps, arm_size)) ? kFastSym : kSymPerWg;
}

template <typename T, bool CFC>
static void launch_symbol_filter(hipStream_t s, unsigned n_wg, size_t smem, unsigned sps, const T* in,
                                 const T* carry, unsigned cap, const float* taps, unsigned arm_size,
                                 const SymRun* runs, unsigned n_runs, SymWg* plan, T* out, CfcDev cfc,
                                 const SymChan* chans = nullptr)
{
    const dim3 grid(n_wg), block(kSymPerWg);
    hipLaunchKernelGGL(k_symf_wg_plan, dim3((n_wg + 255) / 256), dim3(256), 0, s, runs, n_runs, n_wg, sps, arm_size,
                       cfc, plan, chans, symf_per_wg(CFC, sps, arm_size, std::is_same<T, cf>::value));
    if constexpr (!CFC && std::is_same<T, cf>::value) {
        if (symf_long(false, true, sps, arm_size)) {
            const unsigned pitch = symf_long_pitch(arm_size);
            const size_t lds = symf_long_lds(arm_size);
            // (a refusal stays in hipGetLastError(), which the caller reads behind its launches; the launch below is
            // then refused too)
            if (lds > 48 * 1024)
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_symbol_filter_long),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
            hipLaunchKernelGGL(k_symbol_filter_long, grid, dim3(kFastThreads), lds, s, in, carry, cap, taps, arm_size, pitch,
                               plan, out);
            return;
        }
    }
    if constexpr (CFC) {
        if (symf_fast(true, sps, arm_size)) {
#ifdef GR4PM_EXPERIMENTS
            if (timing_skip("symf_fake"))
                hipLaunchKernelGGL(k_symf_fake, grid, dim3(kFastThreads), 0, s, in, plan, out);
            else
#endif
            if (!timing_skip("symf")) {
                static const char* abl_e = gr4pm::experiment_env("GR4PM_SYMF_ABL", true);
                static const int abl = abl_e ? atoi(abl_e) : 0;
                static const unsigned pad = gr4pm::experiment_env_wg("GR4PM_SYMF_PAD", 0u, 0u, 64u * 1024u);
                static const unsigned tiles = gr4pm::experiment_env_wg("GR4PM_SYMF_TILES", 1u, 1u, 64u);
                const dim3 gridf((n_wg + tiles - 1) / tiles);
                SymChan one{}; // the single-channel launch's table entry (unused when `chans` is given)
                one.in = in, one.carry = carry, one.out = out;
                one.segs = cfc.segs, one.seg_incr = cfc.seg_incr, one.seg_counter0 = cfc.seg_counter0;
                one.n_segs = cfc.n_segs;
#define GR4PM_SYMF_LAUNCH(A)                                                                                         \
    do {                                                                                                             \
        if (tiles > 1)                                                                                               \
            hipLaunchKernelGGL((k_symbol_filter_fast<A, true>), gridf, dim3(kFastThreads), pad, s, one, chans, plan, \
                               taps, cfc.ck, cap, n_wg, tiles);                                                      \
        else                                                                                                         \
            hipLaunchKernelGGL((k_symbol_filter_fast<A, false>), gridf, dim3(kFastThreads), pad, s, one, chans, plan, \
                               taps, cfc.ck, cap, n_wg, tiles);                                                      \
    } while (0)
#ifdef GR4PM_EXPERIMENTS
                if (abl == 1) GR4PM_SYMF_LAUNCH(1);
                else if (abl == 2) GR4PM_SYMF_LAUNCH(2);
                else if (abl == 3) GR4PM_SYMF_LAUNCH(3);
                else
#endif
                    GR4PM_SYMF_LAUNCH(0);
                (void)abl;
#undef GR4PM_SYMF_LAUNCH
            }
            return;
        }
    }
    if (sps == 4)
        hipLaunchKernelGGL((k_symbol_filter<T, 4, CFC>), grid, block, smem, s, in, carry, cap, taps, arm_size, sps,
                           plan, out, cfc, chans);
    else if (sps == 2)
        hipLaunchKernelGGL((k_symbol_filter<T, 2, CFC>), grid, block, smem, s, in, carry, cap, taps, arm_size, sps,
                           plan, out, cfc, chans);
    else if (sps == 8)
        hipLaunchKernelGGL((k_symbol_filter<T, 8, CFC>), grid, block, smem, s, in, carry, cap, taps, arm_size, sps,
                           plan, out, cfc, chans);
    else
        hipLaunchKernelGGL((k_symbol_filter<T, 0, CFC>), grid, block, smem, s, in, carry, cap, taps, arm_size, sps,
                           plan, out, cfc, chans);
}

} // namespace
} // namespace gr4pm

using namespace gr4pm;

// ------------------------------------------------------------------ SymbolFilter
struct gr4pm_symbol_filter : gr4pm::hostlogic::SymfHostState { // the tag-driven state: hostlogic/symbol_filter_replay.hpp
    size_t arm_size;
    int item_kind;
    unsigned cap;
    hipStream_t stream;
    DevBuf<float> taps;
    DevBuf<char> carry[2];
    DevBuf<SymRun> runs;
    DevBuf<SymWg> wg_plan;
    int cur = 0;
};

extern "C" {

gr4pm_status gr4pm_symbol_filter_create(const gr4pm_symbol_filter_params* p, gr4pm_symbol_filter** out)
try {
    if (!p || !out || !p->taps) return GR4PM_ERR_INVALID;
    *out = nullptr;
    if (p->samples_per_symbol == 0) { // symbol_filter.hpp:67-69
        set_error("samples_per_symbol cannot be zero");
        return GR4PM_ERR_INVALID;
    }
    if (p->num_arms == 0) { // :71-73
        set_error("num_arms cannot be zero");
        return GR4PM_ERR_INVALID;
    }
    GR4PM_TRY(require_device());
    std::unique_ptr<gr4pm_symbol_filter> h(new (std::nothrow) gr4pm_symbol_filter);
    if (!h) return GR4PM_ERR_NOMEM;
    h->sps = p->samples_per_symbol;
    h->num_arms = p->num_arms;
    h->delay = p->delay;
    h->item_kind = p->item_kind;
    h->stream = static_cast<hipStream_t>(p->stream);
    // polyphase split, :84-90; inner products run over arm 0's length for every arm is NOT
    // what the reference does: each arm has its own length (taps[k], k = j, j+arms, ...)
    h->arm_size = (p->n_taps + p->num_arms - 1) / p->num_arms;
    std::vector<float> taps(h->num_arms * h->arm_size, 0.0f); // shorter arms zero padded
    for (size_t j = 0; j < h->num_arms; ++j) {
        size_t m = 0;
        for (size_t k = j; k < p->n_taps; k += h->num_arms) taps[j * h->arm_size + m++] = p->taps[k];
    }
    const size_t arm0 = (p->n_taps + p->num_arms - 1) / p->num_arms; // _taps[0].size(), :93
    h->cap = static_cast<unsigned>(bit_ceil_sz(std::max<size_t>(arm0, 1)));
    h->reset_clock_phase = (h->sps - (h->delay % h->sps)) % h->sps; // :106-107
    const size_t isz = p->item_kind == 0 ? sizeof(cf) : sizeof(float);
    GR4PM_TRY(h->taps.alloc(taps.size()));
    for (auto& c : h->carry) {
        GR4PM_TRY(c.alloc(h->cap * isz));
        GR4PM_TRY(c.zero(h->stream));
    }
    GR4PM_TRY(h->taps.upload(taps.data(), taps.size(), h->stream));
    return finish_create(h, out, "symbol_filter");
}
GR4PM_ABI_CATCH
void gr4pm_symbol_filter_destroy(gr4pm_symbol_filter* h)
try {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    delete h;
}
GR4PM_ABI_CATCH_VOID
gr4pm_status gr4pm_symbol_filter_reset(gr4pm_symbol_filter* h)
try {
    if (!h) return GR4PM_ERR_INVALID;
    h->clock_phase = 0; // start(), :110
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

} // extern "C"

using hostlogic::SymReplay; // the host replay of symbol_filter.hpp:130-238: hostlogic/symbol_filter_replay.hpp
using hostlogic::symf_replay;

// fuse == nullptr: plain SymbolFilter.  Otherwise the input is rotated by the CFC plan on the fly.
static gr4pm_status symbol_filter_impl(gr4pm_symbol_filter* h, const void* in, size_t n_in, void* out,
                                       size_t out_cap, const gr4pm_tag* tags_in, size_t n_tags_in,
                                       gr4pm_tag* tags_out, size_t tags_cap, size_t* n_tags_out,
                                       size_t* consumed_, size_t* produced_, const CfcDev* fuse)
{
    if (!h || !consumed_ || !produced_) return GR4PM_ERR_INVALID;
    *consumed_ = *produced_ = 0;
    if (n_tags_out) *n_tags_out = 0;
    if (n_in == 0) return GR4PM_OK; // nothing consumed, nothing produced, queued tags keep waiting
    if (!in || !out) {
        set_error("null sample pointer");
        return GR4PM_ERR_INVALID;
    }
    const size_t sps = h->sps;
    SymReplay rp;
    symf_replay(*h, n_in, out_cap, tags_in, n_tags_in, tags_out, tags_cap, rp);
    std::vector<SymRun>& runs = rp.runs;
    const size_t pos = rp.pos, produced = rp.produced, n_pub = rp.n_pub;
    const bool tag_overflow = rp.tag_overflow;
    hipStream_t s = h->stream;
    if (!runs.empty()) {
        unsigned n_wg = 0;
        const unsigned per_wg = symf_per_wg(fuse != nullptr, sps, h->arm_size, h->item_kind == 0);
        for (auto& r : runs) { // workgroups never straddle runs
            r.wg0 = n_wg;
            r.chan = 0;
            n_wg += (r.count + per_wg - 1u) / per_wg;
        }
        GR4PM_TRY(upload_vec(h->runs, runs, s));
        const size_t pitch = (kSymPerWg * sps + h->arm_size) / sps + 2;
        if (h->wg_plan.n < n_wg) GR4PM_TRY(h->wg_plan.alloc(static_cast<size_t>(n_wg) * 2));
        const size_t arm_bytes = ((h->arm_size + 1) & ~size_t{ 1 }) * sizeof(float);
        const unsigned n_runs = static_cast<unsigned>(runs.size());
        if (fuse)
            launch_symbol_filter<cf, true>(
                s, n_wg, pitch * sps * sizeof(cf) + arm_bytes,
                static_cast<unsigned>(sps), static_cast<const cf*>(in),
                reinterpret_cast<const cf*>(h->carry[h->cur].p), h->cap, h->taps.p,
                static_cast<unsigned>(h->arm_size), h->runs.p, n_runs, h->wg_plan.p, static_cast<cf*>(out), *fuse);
        else if (h->item_kind == 0)
            launch_symbol_filter<cf, false>(s, n_wg, pitch * sps * sizeof(cf) + arm_bytes, static_cast<unsigned>(sps),
                                            static_cast<const cf*>(in),
                                            reinterpret_cast<const cf*>(h->carry[h->cur].p), h->cap, h->taps.p,
                                            static_cast<unsigned>(h->arm_size), h->runs.p, n_runs, h->wg_plan.p,
                                            static_cast<cf*>(out), CfcDev{});
        else
            launch_symbol_filter<float, false>(s, n_wg, pitch * sps * sizeof(float) + arm_bytes,
                                               static_cast<unsigned>(sps), static_cast<const float*>(in),
                                               reinterpret_cast<const float*>(h->carry[h->cur].p), h->cap, h->taps.p,
                                               static_cast<unsigned>(h->arm_size), h->runs.p, n_runs, h->wg_plan.p,
                                               static_cast<float*>(out), CfcDev{});
    }
    if (pos > 0) {
        if (fuse)
            hipLaunchKernelGGL(k_update_hist_cfc, dim3((h->cap + 63) / 64), dim3(64), 0, s,
                               static_cast<const cf*>(in), reinterpret_cast<const cf*>(h->carry[h->cur].p),
                               reinterpret_cast<cf*>(h->carry[h->cur ^ 1].p), h->cap, pos, *fuse);
        else if (h->item_kind == 0)
            hipLaunchKernelGGL(k_update_hist<cf>, dim3((h->cap + 63) / 64), dim3(64), 0, s,
                               static_cast<const cf*>(in), reinterpret_cast<const cf*>(h->carry[h->cur].p),
                               reinterpret_cast<cf*>(h->carry[h->cur ^ 1].p), h->cap, pos);
        else
            hipLaunchKernelGGL(k_update_hist<float>, dim3((h->cap + 63) / 64), dim3(64), 0, s,
                               static_cast<const float*>(in),
                               reinterpret_cast<const float*>(h->carry[h->cur].p),
                               reinterpret_cast<float*>(h->carry[h->cur ^ 1].p), h->cap, pos);
        h->cur ^= 1;
    }
    GR4PM_HIP_TRY(hipGetLastError());
    GR4PM_HIP_TRY(final_sync(s));
    *consumed_ = pos;
    *produced_ = produced;
    if (n_tags_out) *n_tags_out = n_pub;
    if (tag_overflow) {
        set_error("tags_cap too small");
        return GR4PM_ERR_OVERFLOW;
    }
    return GR4PM_OK;
}

extern "C" {

gr4pm_status gr4pm_symbol_filter_process(gr4pm_symbol_filter* h, const void* in, size_t n_in, void* out,
                                         size_t out_cap, const gr4pm_tag* tags_in, size_t n_tags_in,
                                         gr4pm_tag* tags_out, size_t tags_cap, size_t* n_tags_out,
                                         size_t* consumed, size_t* produced)
try {
    return symbol_filter_impl(h, in, n_in, out, out_cap, tags_in, n_tags_in, tags_out, tags_cap, n_tags_out,
                              consumed, produced, nullptr);
}
GR4PM_ABI_CATCH

static gr4pm_status cfc_plan_impl(gr4pm_rotator* cfc, size_t n_in, const gr4pm_tag* tags_in,
                                  const uint32_t* tag_channel, size_t n_tags_in, int* plan, bool ring)
{
    if (!cfc || !plan) return GR4PM_ERR_INVALID;
    *plan = -1;
    if (cfc->mode != 1) {
        set_error("fused call needs a CoarseFrequencyCorrection handle");
        return GR4PM_ERR_INVALID;
    }
    if (!tag_channel && cfc->n_channels != 1 && n_tags_in) {
        set_error("tag_channel is required with more than one channel");
        return GR4PM_ERR_INVALID;
    }
    if (n_in == 0) return GR4PM_OK;
    static thread_local hostlogic::RotPlan rp; // (its vectors keep their capacity from call to call)
    GR4PM_TRY(rotator_plan(cfc, n_in, tags_in, tag_channel, n_tags_in, rp, ring)); // checkpoints on the CFC's stream
    *plan = cfc->plan_cur;
    GR4PM_HIP_TRY(final_sync(cfc->stream));
    return GR4PM_OK;
}

gr4pm_status gr4pm_cfc_symbol_filter_plan_channels(gr4pm_rotator* cfc, size_t n_in, const gr4pm_tag* tags_in,
                                                   const uint32_t* tag_channel, size_t n_tags_in, int* plan)
try {
    return cfc_plan_impl(cfc, n_in, tags_in, tag_channel, n_tags_in, plan, true);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_cfc_symbol_filter_plan(gr4pm_rotator* cfc, size_t n_in, const gr4pm_tag* tags_in,
                                          size_t n_tags_in, int* plan)
try {
    if (cfc && cfc->n_channels != 1) {
        set_error("fused call needs a single-channel CoarseFrequencyCorrection (or ..._plan_channels)");
        return GR4PM_ERR_INVALID;
    }
    return gr4pm_cfc_symbol_filter_plan_channels(cfc, n_in, tags_in, nullptr, n_tags_in, plan);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_cfc_symbol_filter_run(gr4pm_rotator* cfc, int plan, gr4pm_symbol_filter* sf,
                                         const gr4pm_c64* in, size_t n_in, gr4pm_c64* out, size_t out_cap,
                                         const gr4pm_tag* tags_in, size_t n_tags_in, gr4pm_tag* tags_out,
                                         size_t tags_cap, size_t* n_tags_out, size_t* consumed, size_t* produced)
try {
    return gr4pm_cfc_symbol_filter_run_channel(cfc, plan, 0, sf, in, n_in, out, out_cap, tags_in, n_tags_in, tags_out,
                                               tags_cap, n_tags_out, consumed, produced);
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_cfc_symbol_filter_run_channel(gr4pm_rotator* cfc, int plan, size_t channel, gr4pm_symbol_filter* sf,
                                                 const gr4pm_c64* in, size_t n_in, gr4pm_c64* out, size_t out_cap,
                                                 const gr4pm_tag* tags_in, size_t n_tags_in, gr4pm_tag* tags_out,
                                                 size_t tags_cap, size_t* n_tags_out, size_t* consumed,
                                                 size_t* produced)
try {
    if (!cfc || !sf || !consumed || !produced) return GR4PM_ERR_INVALID;
    *consumed = *produced = 0;
    if (n_tags_out) *n_tags_out = 0;
    if (sf->item_kind != 0) {
        set_error("fused call needs a complex SymbolFilter");
        return GR4PM_ERR_INVALID;
    }
    if (n_in == 0) return GR4PM_OK;
    if (plan < 0 || plan >= GR4PM_CFC_PLANS || cfc->plans[plan].n_in != n_in) {
        set_error("no rotation plan for this call");
        return GR4PM_ERR_INVALID;
    }
    if (!in || !out) {
        set_error("null sample pointer");
        return GR4PM_ERR_INVALID;
    }
    // the rotation plan covers all n_in items, so the filter must be able to consume them all
    if (out_cap < n_in / sf->sps + n_tags_in + 2) {
        set_error("out_cap too small for a fused call");
        return GR4PM_INSUFFICIENT_OUTPUT_ITEMS;
    }
    const auto& pl = cfc->plans[plan];
    if (channel >= cfc->n_channels || pl.seg_first.size() != cfc->n_channels + 1) {
        set_error("channel %zu outside the rotation plan", channel);
        return GR4PM_ERR_INVALID;
    }
    GR4PM_TRY(cfc_wait_plan(cfc, plan, sf->stream));
    // the channel's own segments (they tile its [0, n_in)); checkpoint slots are plan-wide
    const unsigned first = pl.seg_first[channel];
    CfcDev f;
    f.segs = pl.segs.p + first;
    f.ck = pl.ck.p;
    f.seg_incr = pl.seg_incr.p + first;
    f.seg_counter0 = pl.seg_counter0.p + first;
    f.n_segs = pl.seg_first[channel + 1] - first;
    const gr4pm_status st = symbol_filter_impl(sf, in, n_in, out, out_cap, tags_in, n_tags_in, tags_out, tags_cap,
                                               n_tags_out, consumed, produced, &f);
    if (st == GR4PM_OK && *consumed != n_in) {
        set_error("fused call consumed %zu of %zu items", *consumed, n_in);
        return GR4PM_ERR_INVALID;
    }
    return st;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_cfc_symbol_filter_run_channels(gr4pm_rotator* cfc, int plan, gr4pm_symbol_filter* const* sf,
                                                  size_t n_channels, const gr4pm_c64* in, size_t in_stride, size_t n_in,
                                                  gr4pm_c64* out, size_t out_stride, const gr4pm_tag* const* tags_in,
                                                  const size_t* n_tags_in, gr4pm_tag* const* tags_out, size_t tags_cap,
                                                  size_t* n_tags_out, size_t* produced, const gr4pm_c64* head,
                                                  size_t head_stride, size_t n_head)
try {
    if (!cfc || !sf || !n_tags_in || !tags_in || !tags_out || !n_tags_out || !produced || n_channels == 0)
        return GR4PM_ERR_INVALID;
    for (size_t c = 0; c < n_channels; ++c) n_tags_out[c] = produced[c] = 0;
    if (n_in == 0) return GR4PM_OK;
    if (plan < 0 || plan >= GR4PM_CFC_PLANS || cfc->plans[plan].n_in != n_in) {
        set_error("no rotation plan for this call");
        return GR4PM_ERR_INVALID;
    }
    const auto& pl = cfc->plans[plan];
    if (n_channels != cfc->n_channels || pl.seg_first.size() != cfc->n_channels + 1) {
        set_error("the rotation plan has %zu channels, the call %zu", cfc->n_channels, n_channels);
        return GR4PM_ERR_INVALID;
    }
    if (!in || !out || in_stride + n_head < n_in || (n_head && (!head || head_stride < n_head || n_head > n_in))) {
        set_error("null sample pointer, in_stride + n_head < n_in or a bad head");
        return GR4PM_ERR_INVALID;
    }
    gr4pm_symbol_filter* h0 = sf[0];
    size_t max_tags = 0;
    for (size_t c = 0; c < n_channels; ++c) {
        const gr4pm_symbol_filter* h = sf[c];
        if (!h || h->item_kind != 0 || h->sps != h0->sps || h->arm_size != h0->arm_size || h->cap != h0->cap ||
            h->num_arms != h0->num_arms) {
            set_error("a launch that spans channels needs complex SymbolFilters of one design");
            return GR4PM_ERR_INVALID;
        }
        max_tags = std::max(max_tags, n_tags_in[c]);
    }
    // the rotation plan covers all n_in items, so every filter must be able to consume them all
    if (out_stride < n_in / h0->sps + max_tags + 2) {
        set_error("out_stride too small for a fused call");
        return GR4PM_INSUFFICIENT_OUTPUT_ITEMS;
    }
    // host replay per channel; the runs of all channels in one table
    static_assert(sizeof(SymChan) % 8 == 0 && sizeof(SymRun) % 8 == 0, "table layout");
    std::vector<SymChan> chans(n_channels);
    std::vector<SymRun> runs;
    unsigned n_wg = 0;
    const unsigned per_wg = symf_per_wg(true, h0->sps, h0->arm_size);
    bool overflow = false;
    for (size_t c = 0; c < n_channels; ++c) {
        gr4pm_symbol_filter* h = sf[c];
        SymReplay rp;
        symf_replay(*h, n_in, out_stride, tags_in[c], n_tags_in[c], tags_out[c], tags_cap, rp);
        if (rp.pos != n_in) {
            set_error("fused call consumed %zu of %zu items (channel %zu)", rp.pos, n_in, c);
            return GR4PM_ERR_INVALID;
        }
        overflow |= rp.tag_overflow;
        for (auto& r : rp.runs) { // workgroups never straddle runs
            r.wg0 = n_wg;
            r.chan = static_cast<unsigned>(c);
            n_wg += (r.count + per_wg - 1u) / per_wg;
            runs.push_back(r);
        }
        const unsigned first = pl.seg_first[c];
        SymChan& d = chans[c];
        d.in = reinterpret_cast<const cf*>(in) + c * in_stride;
        d.carry = reinterpret_cast<const cf*>(h->carry[h->cur].p);
        d.carry_next = reinterpret_cast<cf*>(h->carry[h->cur ^ 1].p);
        d.out = reinterpret_cast<cf*>(out) + c * out_stride;
        d.segs = pl.segs.p + first;
        d.seg_incr = pl.seg_incr.p + first;
        d.seg_counter0 = pl.seg_counter0.p + first;
        d.n_segs = pl.seg_first[c + 1] - first;
        d.pad = 0;
        d.n = rp.pos;
        d.head = n_head ? reinterpret_cast<const cf*>(head) + c * head_stride : nullptr;
        d.n_head = n_head;
        h->cur ^= 1;
        produced[c] = rp.produced;
        n_tags_out[c] = rp.n_pub;
    }
    hipStream_t s = h0->stream;
    GR4PM_TRY(cfc_wait_plan(cfc, plan, s));
    const size_t chan_words = n_channels * sizeof(SymChan) / 8, run_words = runs.size() * sizeof(SymRun) / 8;
    cfc->mc_host.resize(chan_words + run_words);
    std::memcpy(cfc->mc_host.data(), chans.data(), chan_words * 8);
    if (run_words) std::memcpy(cfc->mc_host.data() + chan_words, runs.data(), run_words * 8);
    GR4PM_TRY(upload_vec(cfc->mc_tab, cfc->mc_host, s));
    const SymChan* d_chans = reinterpret_cast<const SymChan*>(cfc->mc_tab.p);
    const SymRun* d_runs = reinterpret_cast<const SymRun*>(cfc->mc_tab.p + chan_words);
    CfcDev f{};
    f.ck = pl.ck.p;
    f.n_segs = 1; // per channel from the table
    if (n_wg) {
        if (cfc->mc_wg.n < n_wg) GR4PM_TRY(cfc->mc_wg.alloc(static_cast<size_t>(n_wg) * 2));
        const size_t sps = h0->sps;
        const size_t pitch = (kSymPerWg * sps + h0->arm_size) / sps + 2;
        const size_t arm_bytes = ((h0->arm_size + 1) & ~size_t{ 1 }) * sizeof(float);
        launch_symbol_filter<cf, true>(
            s, n_wg, pitch * sps * sizeof(cf) + arm_bytes,
            static_cast<unsigned>(sps), static_cast<const cf*>(nullptr), static_cast<const cf*>(nullptr), h0->cap,
            h0->taps.p, static_cast<unsigned>(h0->arm_size), d_runs, static_cast<unsigned>(runs.size()), cfc->mc_wg.p,
            static_cast<cf*>(nullptr), f, d_chans);
    }
    hipLaunchKernelGGL(k_update_hist_cfc_channels, dim3((h0->cap + 63) / 64, static_cast<unsigned>(n_channels)),
                       dim3(64), 0, s, d_chans, pl.ck.p, h0->cap);
    GR4PM_HIP_TRY(hipGetLastError());
    GR4PM_HIP_TRY(final_sync(s));
    if (overflow) {
        set_error("tags_cap too small");
        return GR4PM_ERR_OVERFLOW;
    }
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_cfc_symbol_filter_process(gr4pm_rotator* cfc, gr4pm_symbol_filter* sf, const gr4pm_c64* in,
                                             size_t n_in, gr4pm_c64* out, size_t out_cap,
                                             const gr4pm_tag* tags_in, size_t n_tags_in, gr4pm_tag* tags_out,
                                             size_t tags_cap, size_t* n_tags_out, size_t* consumed,
                                             size_t* produced)
try {
    if (!cfc || !sf || !consumed || !produced) return GR4PM_ERR_INVALID;
    *consumed = *produced = 0;
    if (n_tags_out) *n_tags_out = 0;
    if (cfc->stream != sf->stream) {
        set_error("fused call needs the CoarseFrequencyCorrection and the SymbolFilter on one stream");
        return GR4PM_ERR_INVALID;
    }
    if (n_in == 0) return GR4PM_OK;
    if (!in || !out) {
        set_error("null sample pointer");
        return GR4PM_ERR_INVALID;
    }
    if (out_cap < n_in / sf->sps + n_tags_in + 2) { // checked before the plan consumes the tags
        set_error("out_cap too small for a fused call");
        return GR4PM_INSUFFICIENT_OUTPUT_ITEMS;
    }
    if (cfc->n_channels != 1) { // validated before any state is touched
        set_error("fused call needs a single-channel CoarseFrequencyCorrection");
        return GR4PM_ERR_INVALID;
    }
    int plan = -1;
    gr4pm_status st;
    {
        // same stream: the filter queues up behind the checkpoints
        // (one stream, nothing in between: the current plan set is reused, no ring)
        DeferredSyncScope defer;
        st = cfc_plan_impl(cfc, n_in, tags_in, nullptr, n_tags_in, &plan, false);
    }
    if (st != GR4PM_OK) return st;
    return gr4pm_cfc_symbol_filter_run(cfc, plan, sf, in, n_in, out, out_cap, tags_in, n_tags_in, tags_out,
                                       tags_cap, n_tags_out, consumed, produced);
}
GR4PM_ABI_CATCH

} // extern "C"
