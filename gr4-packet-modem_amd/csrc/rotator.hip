// rotator.hip -- Rotator (rotator.hpp:44-65) and CoarseFrequencyCorrection
// (coarse_frequency_correction.hpp:50-98): y = x * e; e *= e_incr; renormalise every 512.
// The phasor recurrence is order dependent: it runs serially per independent segment (one lane each) and leaves
// checkpoints, from which every sample is rotated in parallel.  (Conventions of the stream blocks: stream_blocks.hpp.)
#include "rotator.hpp"

namespace gr4pm {
namespace {

// cmul(a, b) as three packed instructions: (a.x b.x, a.x b.y), (a.y b.y, a.y b.x), then
// (t.x - u.x, t.y + u.y) -- the same four products and two sums, each rounded once
__device__ __forceinline__ __attribute__((unused)) cf cmul_pk(cf a, cf b)
{
    cf t, u, r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(t) : "v"(a), "v"(b));
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[1,0]" : "=v"(u) : "v"(a), "v"(b));
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,0]" : "=v"(r) : "v"(t), "v"(u));
    return r;
}

// kRotChunk steps e *= inc without renormalisation, three packed instructions a step:
//   a = (e.x * inc.x, e.x * inc.y)   b = (e.y * inc.y, e.y * inc.x)   e = (a.x - b.x, a.y + b.y)
// which are exactly the four products and two sums of cmul(), each rounded once (the sign of
// b.x is an input modifier).  No s_nop between a packed result and its packed consumer: the hardware
// interlocks (hipcc pads such pairs because it takes op_sel_hi of a VOP3P source for a dst_sel; the
// correlator's cmul has run them unpadded, bit-exact, since round 1).  hipcc itself spends seven instructions
// and four dependent levels a step on the same arithmetic (it builds both a + b and a - b and moves halves around).
__device__ __forceinline__ cf rot_chunk_pk(cf e, cf inc)
{
    static_assert(kRotChunk == 8, "eight unrolled steps below");
    cf a, b;
#define GR4PM_ROT_STEP                                                  \
    "v_pk_mul_f32 %[a], %[e], %[i] op_sel_hi:[0,1]\n"                   \
    "v_pk_mul_f32 %[b], %[e], %[i] op_sel:[1,1] op_sel_hi:[1,0]\n"      \
    "v_pk_add_f32 %[e], %[a], %[b] neg_lo:[0,1] neg_hi:[0,0]\n"
    asm volatile(GR4PM_ROT_STEP GR4PM_ROT_STEP GR4PM_ROT_STEP GR4PM_ROT_STEP GR4PM_ROT_STEP GR4PM_ROT_STEP
                     GR4PM_ROT_STEP GR4PM_ROT_STEP
                 : [e] "+v"(e), [a] "=&v"(a), [b] "=&v"(b)
                 : [i] "v"(inc));
#undef GR4PM_ROT_STEP
    return e;
}

// Measured, not adopted (round 3): four chains per lane, interleaved (k_rot_checkpoints4: a quarter of the waves).
// A chain's step is NOT latency-bound on this chip: the four-chain kernel took 3.7 x the time of the one-chain kernel
// (1.49 against 0.40 ms for 10 004 packet segments, with or without the checkpoint stores) -- each packed instruction
// costs the same ~5 ns whether its neighbours depend on it or not, and the pipelined receiver lost 6 % (stage latency).
// serial: one lane per segment, phasor checkpoints every kRotChunk samples.  The chain of
// dependent complex multiplies is the whole cost, so the loop body is kept to exactly that.
// Register budget: at most 32 VGPRs, on purpose.  These waves live for half a millisecond; a SIMD that runs two
// correlator waves (2 x 240 registers) has exactly 32 left, so a wave of this kernel fits BESIDE them instead of keeping
// the next correlator workgroup off its CU (HISTORY.md section 9).  Hence: segment fields are re-read where they are
// needed instead of kept, chunk counts are 32 bit (a segment is shorter than 2^35 items), one running pointer.
__device__ __forceinline__ void rot_checkpoints_generic(unsigned lane_seg, const RotSeg* __restrict__ segs, unsigned n_segs,
                                                        const RotState* __restrict__ state,
                                                        RotState* __restrict__ state_next, cf* __restrict__ ck,
                                                        cf* __restrict__ seg_incr, unsigned* __restrict__ seg_counter0,
                                                        const unsigned* __restrict__ order)
{
    if (lane_seg >= n_segs) return;
    // order[]: the segments by descending length, so that the long ones (a stream with missed detections) share
    // waves -- a wave lives as long as its longest lane (see costas_process_impl); the array itself stays sorted by
    // position (k_rot_apply and the fused symbol filter search it)
    const unsigned s = order[lane_seg];
    const RotSeg* gp = segs + s;
    cf e, inc;
    unsigned counter;
    if (gp->mode == 2) {
        // a fixed point of the recurrence (see gr4pm_rotator::fixed): no chain; k_rot_const_fill writes the checkpoints
        seg_incr[s] = gp->incr;
        seg_counter0[s] = 0;
        if (gp->last) {
            RotState st;
            st.exp = gp->exp0;
            st.incr = gp->incr;
            st.counter = 0; // (irrelevant while the phasor is fixed; the next set_freq() resets it)
            st.pad = 0;
            state_next[gp->channel] = st;
        }
        return;
    }
    if (gp->mode == 0) {
        const RotState* st = state + gp->channel;
        e = st->exp;
        inc = st->incr;
        counter = st->counter;
    } else {
        e = gp->exp0;
        inc = gp->incr;
        counter = 0;
    }
    seg_incr[s] = inc;
    seg_counter0[s] = counter;
    cf* ckp = ck + gp->ck0;
    unsigned left = static_cast<unsigned>(gp->len / kRotChunk);
    // Round 6 (see k_rot_checkpoints_fresh): whole periods of 64 chunks in a loop without per-chunk decisions.  The
    // renormalisation falls into every 64th chunk, always the same one: the chunk loop below runs up to it (`lead` chunks),
    // then every period is that chunk item by item + 63 plain chunks under a scalar counter; what is left (less than a
    // period) goes through the chunk loop again.  Checkpoints leave 8 bytes at a time here: a continuation's slot has any
    // alignment, and there is one such segment per channel.
    const unsigned lead = ((512u - (counter & 511u)) - 1u) / kRotChunk; // plain chunks in front of the renormalising one
    const bool periods = left > lead && left - lead >= 64u;
    for (int phase = 0; phase < 2; ++phase) {
    const unsigned stop = phase == 0 && periods ? left - lead : 0u; // chunks still to do when this phase ends
    while (left != stop) {
        // (rounds 3 - 5 took four chunks per pass here while no renormalisation fell into them, with 16-byte stores where the
        // slot was aligned -- decided per lane; the periods below have taken that over, this loop sees less than 64 chunks)
        *ckp++ = e;
        --left;
        if ((counter & 511u) < 512u - kRotChunk) { // no renormalisation inside this chunk
            e = rot_chunk_pk(e, inc);
            counter += kRotChunk;
        } else { // one chunk in 64: rolled, ONE instance of the renormalisation's double-precision square root
#pragma unroll 1
            for (unsigned j = 0; j < kRotChunk; ++j) rot_step(e, inc, counter);
        }
    }
    if (phase == 0 && periods) {
        for (; left >= 64u; left -= 64u) {
            *ckp++ = e;
#pragma unroll 1
            for (unsigned j = 0; j < kRotChunk; ++j) rot_step(e, inc, counter); // the period's renormalising chunk
#pragma unroll 1
            for (int k = 0; k < 63; ++k) {
                *ckp++ = e;
                e = rot_chunk_pk(e, inc);
            }
            counter += 63 * kRotChunk;
        }
    }
    } // phases
    gp = segs + s; // (recomputed: one register kept across the loop instead of two)
    const unsigned rem = static_cast<unsigned>(gp->len) & (kRotChunk - 1);
    if (rem) {
        *ckp = e;
        for (unsigned j = 0; j < rem; ++j) rot_step(e, inc, counter);
    }
    if (gp->last) {
        RotState st;
        st.exp = e;
        st.incr = inc;
        st.counter = counter;
        st.pad = 0;
        state_next[gp->channel] = st; // (another row of the ring: another lane may still have to read `state`)
    }
}
__global__ __launch_bounds__(64) void k_rot_checkpoints(const RotSeg* __restrict__ segs, unsigned n_segs,
                                                        const RotState* __restrict__ state,
                                                        RotState* __restrict__ state_next, cf* __restrict__ ck,
                                                        cf* __restrict__ seg_incr, unsigned* __restrict__ seg_counter0,
                                                        const unsigned* __restrict__ order)
{
    __builtin_amdgcn_s_setprio(GR4PM_ROT_PRIO); // latency-bound, few waves
    rot_checkpoints_generic(blockIdx.x * blockDim.x + threadIdx.x, segs, n_segs, state, state_next, ck, seg_incr, seg_counter0,
                            order);
}

// Round 6: the segments that START at a set_freq event (mode 1; the host gives them an even checkpoint slot) in a loop
// without per-chunk decisions.  tools/lone_wave_issue.hip: the chain's three packed instructions cost a lone wave 5.2 core
// clocks each, 6.5 ns a step -- the kernel above takes 12 - 16: every chunk of eight steps it tests the renormalisation
// counter and the slot's alignment per LANE (the lanes of a wave disagree, so both paths run), and the renormalisation's
// chunk goes through a rolled loop.  A fresh segment's counter starts at 0: a period of 512 steps is 31 pairs of chunks
// (one 16-byte store each), one more chunk, seven plain steps and the step that renormalises -- the same operations in
// the same order, under a SCALAR loop counter.  The continuations (mode 0: any counter, any alignment) stay above.
__device__ __forceinline__ void rot_checkpoints_fresh(unsigned lane_seg, const RotSeg* __restrict__ segs, unsigned n_segs,
                                                      RotState* __restrict__ state_next, cf* __restrict__ ck,
                                                      cf* __restrict__ seg_incr, unsigned* __restrict__ seg_counter0,
                                                      const unsigned* __restrict__ order)
{
    if (lane_seg >= n_segs) return;
    const unsigned s = order[lane_seg];
    const RotSeg* gp = segs + s;
    if (gp->mode == 2) { // a fixed point of the recurrence: no chain (k_rot_checkpoints)
        seg_incr[s] = gp->incr;
        seg_counter0[s] = 0;
        if (gp->last) {
            RotState st;
            st.exp = gp->exp0;
            st.incr = gp->incr;
            st.counter = 0;
            st.pad = 0;
            state_next[gp->channel] = st;
        }
        return;
    }
    cf e = gp->exp0;
    const cf inc = gp->incr;
    seg_incr[s] = inc;
    seg_counter0[s] = 0;
    float4* ckp = reinterpret_cast<float4*>(ck + gp->ck0); // (an even slot)
    unsigned chunks = static_cast<unsigned>(gp->len / kRotChunk);
    unsigned counter = 0;
    constexpr unsigned kPeriodChunks = 512 / kRotChunk;
    for (; chunks >= kPeriodChunks; chunks -= kPeriodChunks) {
#pragma unroll 1
        for (int pair = 0; pair < static_cast<int>(kPeriodChunks / 2) - 1; ++pair) {
            const cf e0 = e;
            e = rot_chunk_pk(e, inc);
            *ckp++ = make_float4(e0.x, e0.y, e.x, e.y);
            e = rot_chunk_pk(e, inc);
        }
        const cf e0 = e;
        e = rot_chunk_pk(e, inc);
        *ckp++ = make_float4(e0.x, e0.y, e.x, e.y);
        counter += 512 - kRotChunk;
#pragma unroll 1
        for (unsigned j = 0; j < kRotChunk; ++j) rot_step(e, inc, counter); // (its last step renormalises)
    }
    // less than a period is left: no renormalisation any more
    for (; chunks >= 2; chunks -= 2) {
        const cf e0 = e;
        e = rot_chunk_pk(e, inc);
        *ckp++ = make_float4(e0.x, e0.y, e.x, e.y);
        e = rot_chunk_pk(e, inc);
        counter += 2 * kRotChunk;
    }
    cf* ck1 = reinterpret_cast<cf*>(ckp);
    if (chunks) {
        *ck1++ = e;
        e = rot_chunk_pk(e, inc);
        counter += kRotChunk;
    }
    gp = segs + s; // (recomputed: one register kept across the loops instead of two)
    const unsigned rem = static_cast<unsigned>(gp->len) & (kRotChunk - 1);
    if (rem) {
        *ck1 = e;
        for (unsigned j = 0; j < rem; ++j) rot_step(e, inc, counter);
    }
    if (gp->last) {
        RotState st;
        st.exp = e;
        st.incr = inc;
        st.counter = counter;
        st.pad = 0;
        state_next[gp->channel] = st;
    }
}

__global__ __launch_bounds__(64) void k_rot_checkpoints_fresh(const RotSeg* __restrict__ segs, unsigned n_segs,
                                                              RotState* __restrict__ state_next, cf* __restrict__ ck,
                                                              cf* __restrict__ seg_incr, unsigned* __restrict__ seg_counter0,
                                                              const unsigned* __restrict__ order)
{
    __builtin_amdgcn_s_setprio(GR4PM_ROT_PRIO); // latency-bound, few waves
    rot_checkpoints_fresh(blockIdx.x * blockDim.x + threadIdx.x, segs, n_segs, state_next, ck, seg_incr, seg_counter0, order);
}
// one launch for a whole plan on one stream: the first `fresh_blocks` workgroups take the n_fresh event-started entries of
// order[], the others the continuations behind them -- side by side, as in the one kernel of rounds 1 - 5 (two launches on
// one stream would run the continuation's chain BEHIND the others: 240 + 390 us per 2^28 samples where one kernel took 420)
__global__ __launch_bounds__(64) void k_rot_checkpoints_both(const RotSeg* __restrict__ segs, unsigned n_fresh,
                                                             unsigned fresh_blocks, unsigned n_rest,
                                                             const RotState* __restrict__ state,
                                                             RotState* __restrict__ state_next, cf* __restrict__ ck,
                                                             cf* __restrict__ seg_incr, unsigned* __restrict__ seg_counter0,
                                                             const unsigned* __restrict__ order)
{
    __builtin_amdgcn_s_setprio(GR4PM_ROT_PRIO); // latency-bound, few waves
    if (blockIdx.x < fresh_blocks) // (uniform)
        rot_checkpoints_fresh(blockIdx.x * blockDim.x + threadIdx.x, segs, n_fresh, state_next, ck, seg_incr, seg_counter0, order);
    else
        rot_checkpoints_generic((blockIdx.x - fresh_blocks) * blockDim.x + threadIdx.x, segs, n_rest, state, state_next, ck,
                                seg_incr, seg_counter0, order + n_fresh);
}

// (tests only: GR4PM_TEST_ROT_DELAY_US) keeps a stream busy for `us` microseconds
__global__ void k_test_delay(unsigned us)
{
    const unsigned long long t0 = wall_clock64(); // 100 MHz
    while (wall_clock64() - t0 < 100ull * us) __builtin_amdgcn_s_sleep(64);
}

// the checkpoints of the segments whose phasor is a fixed point of the recurrence (RotSeg::mode == 2): the constant
__global__ __launch_bounds__(256) void k_rot_const_fill(const RotSeg* __restrict__ segs, const unsigned* __restrict__ list,
                                                        cf* __restrict__ ck)
{
    const RotSeg* g = segs + list[blockIdx.y];
    const unsigned long long n = (g->len + kRotChunk - 1) / kRotChunk;
    const cf e = g->exp0;
    cf* dst = ck + g->ck0;
    for (unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
         i += static_cast<unsigned long long>(gridDim.x) * blockDim.x)
        dst[i] = e;
}

// parallel: one lane per SAMPLE (coalesced 8-byte accesses); the lane replays at most
// kRotChunk-1 steps of the recurrence from its chunk's checkpoint, in the reference's order
__global__ __launch_bounds__(256) void k_rot_apply(const RotSeg* __restrict__ segs, unsigned n_segs,
                                                   const cf* __restrict__ ck, const cf* __restrict__ seg_incr,
                                                   const unsigned* __restrict__ seg_counter0,
                                                   const cf* __restrict__ in, cf* __restrict__ out,
                                                   size_t stride)
{
    // blockIdx.y = segment; grid-stride over the segment's samples
    const RotSeg g = segs[blockIdx.y];
    const cf inc = seg_incr[blockIdx.y];
    const unsigned c0 = seg_counter0[blockIdx.y];
    const size_t base = static_cast<size_t>(g.channel) * stride + g.start;
    for (unsigned long long j = static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x; j < g.len;
         j += static_cast<unsigned long long>(gridDim.x) * blockDim.x) {
        const unsigned long long c = j / kRotChunk;
        const unsigned steps = static_cast<unsigned>(j - c * kRotChunk);
        cf e = ck[g.ck0 + c];
        unsigned counter = c0 + static_cast<unsigned>(c * kRotChunk);
        for (unsigned t = 0; t < steps; ++t) rot_step(e, inc, counter);
        out[base + j] = cmul(in[base + j], e);
    }
    (void)n_segs;
}

} // namespace
} // namespace gr4pm

using namespace gr4pm;

// ------------------------------------------------------------------------ Rotator / CFC
// the handle's own streams idle (the chains of ring plans run there)
static void rotator_sync_own_streams(gr4pm_rotator* h)
{
    for (hipStream_t a : h->aux)
        if (a) (void)hipStreamSynchronize(a);
}

static gr4pm_status rotator_reset_impl(gr4pm_rotator* h)
{
    rotator_sync_own_streams(h);
    h->last_async_plan = -1;
    for (auto& y : h->sync) y.async = false;
    std::vector<RotState> st(h->n_channels);
    for (auto& s : st) {
        s.exp = { 1.0f, 0.0f };
        s.counter = 0;
        s.pad = 0;
        if (h->mode == 0) // rotator.hpp:44-48 settingsChanged + :50-54 start
            s.incr = { std::cos(h->phase_incr), std::sin(h->phase_incr) };
        else
            s.incr = { 1.0f, 0.0f };
    }
    GR4PM_HIP_TRY(hipMemcpyAsync(h->state.p, st.data(), st.size() * sizeof(RotState), hipMemcpyHostToDevice,
                                 h->stream));
    GR4PM_HIP_TRY(hipStreamSynchronize(h->stream));
    h->st_cur = 0;
    hostlogic::rot_reset(*h, st[0].exp, st[0].incr);
    return GR4PM_OK;
}

extern "C" {

gr4pm_status gr4pm_rotator_create(const gr4pm_rotator_params* p, gr4pm_rotator** out)
try {
    if (!p || !out || p->n_channels == 0 || (p->mode != 0 && p->mode != 1)) return GR4PM_ERR_INVALID;
    *out = nullptr;
    GR4PM_TRY(require_device());
    std::unique_ptr<gr4pm_rotator> h(new (std::nothrow) gr4pm_rotator);
    if (!h) return GR4PM_ERR_NOMEM;
    h->mode = p->mode;
    h->phase_incr = p->phase_incr;
    h->delay = p->delay;
    h->n_channels = p->n_channels;
    h->stream = static_cast<hipStream_t>(p->stream);
    {
        const char* q = getenv("GPU_MAX_HW_QUEUES");
        const int hw_queues = q ? atoi(q) : 4;
        h->async_policy = getenv("GR4PM_ROT_SERIAL") ? -1 : getenv("GR4PM_ROT_ASYNC") ? 1 : hw_queues >= 8 ? 0 : -1;
        if (const char* d = getenv("GR4PM_TEST_ROT_DELAY_US")) h->test_delay_us = static_cast<unsigned>(std::max(0, atoi(d)));
    }
    GR4PM_TRY(h->state.alloc(static_cast<size_t>(gr4pm_rotator::kStates) * h->n_channels));
    GR4PM_TRY(rotator_reset_impl(h.get()));
    return finish_create(h, out, "rotator");
}
GR4PM_ABI_CATCH
void gr4pm_rotator_destroy(gr4pm_rotator* h)
try {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    rotator_sync_own_streams(h);
    delete h; // (~gr4pm_rotator releases the events and streams)
}
GR4PM_ABI_CATCH_VOID
gr4pm_status gr4pm_rotator_reset(gr4pm_rotator* h)
try {
    return h ? rotator_reset_impl(h) : GR4PM_ERR_INVALID;
}
GR4PM_ABI_CATCH

} // extern "C"

// host replay of the tag-driven control flow (hostlogic::rot_plan) + the serial phasor checkpoints; leaves the segment
// table, checkpoints, increments and counters of this call on the device (h->plans[h->plan_cur])
// ring: the plan goes to the next set of the ring (callers that keep several plans alive:
// gr4pm_cfc_symbol_filter_plan*); otherwise the current set is reused.  When the ring is used for
// the first time every set gets the capacity of the first plan, so that no later call of a
// steady stream has to allocate.
// The host half of the carried state (pending frequency, fixed-point flags) comes back in rp.carried; the handle takes it
// over, with plan_cur and st_cur, where this function returns GR4PM_OK -- behind the allocations, uploads and launches
// that can still fail: a call that fails leaves all three as it found them, in step with the device's RotState.
gr4pm_status gr4pm::rotator_plan(gr4pm_rotator* h, size_t n, const gr4pm_tag* tags, const uint32_t* tag_channel,
                                 size_t n_tags, hostlogic::RotPlan& rp, bool ring)
{
    static const bool no_fixed = getenv("GR4PM_ROT_NO_FIXED_POINT") != nullptr; // A/B: every segment as a chain
    static const bool no_sort = gr4pm::experiment_env("GR4PM_ROT_NO_SORT", false) != nullptr;
    hostlogic::rot_plan(*h, n, tags, tag_channel, n_tags, no_fixed, no_sort, rp);
    const std::vector<RotSeg>& segs = rp.segs;
    const unsigned ck = rp.ck_total;
    const size_t n_const = rp.const_list.size();
    hipStream_t s = h->stream;
    const unsigned n_segs = static_cast<unsigned>(segs.size());
    const int plan = ring ? (h->plan_cur + 1) % GR4PM_CFC_PLANS : h->plan_cur;
    if (ring) {
        if (!h->ring_sized) {
            h->ring_sized = true;
            for (auto& q : h->plans) {
                if (q.ck.n < ck) GR4PM_TRY(q.ck.alloc(static_cast<size_t>(ck) * 2));
                if (q.seg_incr.n < n_segs) {
                    GR4PM_TRY(q.seg_incr.alloc(n_segs * 2));
                    GR4PM_TRY(q.seg_counter0.alloc(n_segs * 2));
                }
                if (q.segs.n < n_segs) GR4PM_TRY(q.segs.alloc(n_segs * 2));
                GR4PM_TRY(q.segs.reserve_stage(n_segs));
                if (q.order.n < n_segs) GR4PM_TRY(q.order.alloc(n_segs * 2));
                GR4PM_TRY(q.order.reserve_stage(n_segs));
                if (q.const_list.n < n_segs) GR4PM_TRY(q.const_list.alloc(n_segs * 2));
                GR4PM_TRY(q.const_list.reserve_stage(n_segs));
            }
        }
    }
    auto& pl = h->plans[plan];
    pl.n_segs = n_segs;
    pl.n_in = n;
    pl.seg_first = rp.seg_first;
    GR4PM_TRY(upload_vec(pl.segs, segs, s));
    if (pl.ck.n < ck) GR4PM_TRY(pl.ck.alloc(static_cast<size_t>(ck) * 2));
    if (pl.seg_incr.n < n_segs) {
        GR4PM_TRY(pl.seg_incr.alloc(n_segs * 2));
        GR4PM_TRY(pl.seg_counter0.alloc(n_segs * 2));
    }
    // order[]: indep | writer | dep, each part by descending length (hostlogic::RotPlan)
    const unsigned n_indep = rp.n_indep, n_writer = rp.n_writer;
    const bool dep_writes_state = rp.dep_writes_state;
    GR4PM_TRY(upload_vec(pl.order, rp.order, s));
    if (n_const) GR4PM_TRY(upload_vec(pl.const_list, rp.const_list, s));
    const unsigned long long longest_const = rp.longest_const;
    const RotState* st_in = h->state.p + static_cast<size_t>(h->st_cur) * h->n_channels;
    const int st_next = (h->st_cur + 1) % gr4pm_rotator::kStates;
    RotState* st_out = h->state.p + static_cast<size_t>(st_next) * h->n_channels;
    static const unsigned wg = gr4pm::experiment_env_wg("GR4PM_ROT_WG", 64u, 1u, 64u); // __launch_bounds__(64)
    // the entries of order[] in front of n_indep + n_writer start at an event (or are fixed points): k_rot_checkpoints_fresh;
    // GR4PM_ROT_GENERIC=1: the one kernel of rounds 1 - 5 for everything (A/B)
    static const bool generic_only = getenv("GR4PM_ROT_GENERIC") != nullptr;
    auto launch_chains = [&](hipStream_t on, unsigned first, unsigned count) {
        if (!count || timing_skip("rot")) return; // GR4PM_TIMING_SKIP: what a kernel costs the pipeline (results are garbage)
        const unsigned n_fresh = generic_only ? 0u : n_indep + n_writer;
        const unsigned fresh = first < n_fresh ? std::min(count, n_fresh - first) : 0u;
        if (fresh && count > fresh) {
            const unsigned fresh_blocks = grid_for(fresh, wg);
            hipLaunchKernelGGL(k_rot_checkpoints_both, dim3(fresh_blocks + grid_for(count - fresh, wg)), dim3(wg), 0, on,
                               pl.segs.p, fresh, fresh_blocks, count - fresh, st_in, st_out, pl.ck.p, pl.seg_incr.p,
                               pl.seg_counter0.p, pl.order.p + first);
        } else if (fresh) {
            hipLaunchKernelGGL(k_rot_checkpoints_fresh, dim3(grid_for(fresh, wg)), dim3(wg), 0, on, pl.segs.p, fresh, st_out,
                               pl.ck.p, pl.seg_incr.p, pl.seg_counter0.p, pl.order.p + first);
        } else {
            hipLaunchKernelGGL(k_rot_checkpoints, dim3(grid_for(count, wg)), dim3(wg), 0, on, pl.segs.p, count, st_in, st_out,
                               pl.ck.p, pl.seg_incr.p, pl.seg_counter0.p, pl.order.p + first);
        }
    };
    auto launch_const_fill = [&](hipStream_t on) {
        if (!n_const) return;
        const unsigned gx = static_cast<unsigned>(std::min<unsigned long long>((longest_const / kRotChunk + 255) / 256 + 1, 2048));
        for (size_t first = 0; first < n_const; first += 65535) {
            const unsigned rows = static_cast<unsigned>(std::min<size_t>(65535, n_const - first));
            hipLaunchKernelGGL(k_rot_const_fill, dim3(gx, rows), dim3(256), 0, on, pl.segs.p, pl.const_list.p + first, pl.ck.p);
        }
    };
    // (tests: GR4PM_TEST_ROT_DELAY_US holds every chain kernel of such a plan back by that long, so that a consumer that
    // does not wait for the plan's events reads checkpoints that are not there yet)
    const unsigned test_delay_us = h->test_delay_us;
    const unsigned long long longest_chain = rp.longest_chain;
    const bool side_by_side = ring && (h->async_policy > 0 || (h->async_policy == 0 && longest_chain >= gr4pm_rotator::kAsyncMinItems));
    auto& sy = h->sync[plan];
    if (side_by_side) {
        if (!h->async_ready) { // the handle's own streams (at the priority of the one it was given) and the plans' events
            int prio = 0;
            GR4PM_HIP_TRY(hipStreamGetPriority(s, &prio));
            for (auto& a : h->aux) GR4PM_HIP_TRY(hipStreamCreateWithPriority(&a, hipStreamNonBlocking, prio));
            for (auto& y : h->sync) {
                GR4PM_HIP_TRY(hipEventCreateWithFlags(&y.up, hipEventDisableTiming));
                GR4PM_HIP_TRY(hipEventCreateWithFlags(&y.indep, hipEventDisableTiming));
                GR4PM_HIP_TRY(hipEventCreateWithFlags(&y.writer, hipEventDisableTiming));
                GR4PM_HIP_TRY(hipEventCreateWithFlags(&y.dep, hipEventDisableTiming));
            }
            h->async_ready = true;
        }
        constexpr int K = gr4pm_rotator::kAux;
        const int turn = plan % K;
        hipStream_t s_indep = h->aux[turn], s_writer = h->aux[K + turn], s_dep = h->aux[2 * K + turn];
        GR4PM_HIP_TRY(hipEventRecord(sy.up, s)); // tables of this plan on the device, and everything `s` carried before
        GR4PM_HIP_TRY(hipStreamWaitEvent(s_indep, sy.up, 0));
        if (test_delay_us) hipLaunchKernelGGL(k_test_delay, dim3(1), dim3(64), 0, s_indep, test_delay_us);
        launch_chains(s_indep, 0, n_indep);
        launch_const_fill(s_indep);
        GR4PM_HIP_TRY(hipEventRecord(sy.indep, s_indep));
        GR4PM_HIP_TRY(hipStreamWaitEvent(s_writer, sy.up, 0));
        if (test_delay_us) hipLaunchKernelGGL(k_test_delay, dim3(1), dim3(64), 0, s_writer, test_delay_us / 3);
        launch_chains(s_writer, n_indep, n_writer);
        GR4PM_HIP_TRY(hipEventRecord(sy.writer, s_writer));
        // the continuations read the carried phasor: behind the kernels of the plan before that wrote it
        GR4PM_HIP_TRY(hipStreamWaitEvent(s_dep, sy.up, 0));
        if (h->last_async_plan >= 0) {
            const auto& before = h->sync[h->last_async_plan];
            GR4PM_HIP_TRY(hipStreamWaitEvent(s_dep, before.writer, 0));
            if (before.dep_writes_state) GR4PM_HIP_TRY(hipStreamWaitEvent(s_dep, before.dep, 0));
        }
        if (test_delay_us) hipLaunchKernelGGL(k_test_delay, dim3(1), dim3(64), 0, s_dep, test_delay_us / 2);
        launch_chains(s_dep, n_indep + n_writer, n_segs - n_indep - n_writer);
        GR4PM_HIP_TRY(hipEventRecord(sy.dep, s_dep));
        sy.async = true;
        sy.dep_writes_state = dep_writes_state;
        h->last_async_plan = plan;
    } else {
        if (h->last_async_plan >= 0) { // (a plain call behind ring plans: their kernels wrote the state this one reads)
            GR4PM_HIP_TRY(hipStreamWaitEvent(s, h->sync[h->last_async_plan].writer, 0));
            GR4PM_HIP_TRY(hipStreamWaitEvent(s, h->sync[h->last_async_plan].dep, 0));
            h->last_async_plan = -1;
        }
        launch_chains(s, 0, n_segs);
        launch_const_fill(s);
        sy.async = false;
    }
    GR4PM_HIP_TRY(hipGetLastError());
    std::swap(h->carried, rp.carried);
    h->plan_cur = plan;
    h->st_cur = st_next;
    return GR4PM_OK;
}

// the chains of a ring plan run on the rotator's own streams (gr4pm_rotator::PlanSync): what reads its checkpoints waits
// for them on its own stream, not on the host
gr4pm_status gr4pm::cfc_wait_plan(gr4pm_rotator* cfc, int plan, hipStream_t consumer)
{
    const auto& y = cfc->sync[plan];
    if (!y.async) return GR4PM_OK;
    GR4PM_HIP_TRY(hipStreamWaitEvent(consumer, y.indep, 0));
    GR4PM_HIP_TRY(hipStreamWaitEvent(consumer, y.writer, 0));
    GR4PM_HIP_TRY(hipStreamWaitEvent(consumer, y.dep, 0));
    return GR4PM_OK;
}

extern "C" {

gr4pm_status gr4pm_rotator_process(gr4pm_rotator* h, const gr4pm_c64* in, size_t stride, size_t n,
                                   gr4pm_c64* out, const gr4pm_tag* tags, const uint32_t* tag_channel,
                                   size_t n_tags)
try {
    if (!h) return GR4PM_ERR_INVALID;
    if (n == 0) return GR4PM_OK; // an empty chunk is legal (and may come with null pointers)
    if (!in || !out) {
        set_error("null sample pointer");
        return GR4PM_ERR_INVALID;
    }
    static thread_local hostlogic::RotPlan rp; // (its vectors keep their capacity from call to call)
    GR4PM_TRY(rotator_plan(h, n, tags, tag_channel, n_tags, rp));
    const std::vector<RotSeg>& segs = rp.segs;
    hipStream_t s = h->stream;
    const unsigned n_segs = static_cast<unsigned>(segs.size());
    {
        size_t longest = 0;
        for (const auto& g : segs) longest = std::max<size_t>(longest, g.len);
        const unsigned gx = static_cast<unsigned>(std::min<size_t>((longest + 255) / 256, 4096));
        // grid.y = segment (at most 65535 per launch)
        for (unsigned s0 = 0; s0 < n_segs; s0 += 65535u) {
            const unsigned ns = std::min(65535u, n_segs - s0);
            const auto& pl = h->plans[h->plan_cur];
            hipLaunchKernelGGL(k_rot_apply, dim3(gx, ns), dim3(256), 0, s, pl.segs.p + s0, ns, pl.ck.p,
                               pl.seg_incr.p + s0, pl.seg_counter0.p + s0, reinterpret_cast<const cf*>(in),
                               reinterpret_cast<cf*>(out), stride);
        }
    }
    GR4PM_HIP_TRY(hipGetLastError());
    GR4PM_HIP_TRY(hipStreamSynchronize(s));
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

} // extern "C"
