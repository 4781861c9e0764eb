// rotator.hpp -- what the fused symbol filter (stream_blocks.hip) needs of the rotator (rotator.hip): the carried
// phasor state, one step of its recurrence, the handle with its ring of plans, and the two host functions that make a
// plan and make a consumer's stream wait for it.
#pragma once
#include "stream_blocks.hpp"
#include "hostlogic/rotator_plan.hpp"

namespace gr4pm {
namespace {

struct RotState {
    cf exp, incr;
    unsigned counter;
    unsigned pad;
};
using hostlogic::RotSeg; // the segment table and who makes it: hostlogic/rotator_plan.hpp
using hostlogic::kRotChunk;

// one step of the phasor recurrence (rotator.hpp:58-63): e *= inc; renormalise when the
// incremented counter is a multiple of 512
__device__ __forceinline__ void rot_step(cf& e, cf inc, unsigned& counter)
{
    e = cmul(e, inc);
    if ((++counter & 511u) == 0) {
        const float r = hypot_like_glibc(e.x, e.y);
        e = { e.x / r, e.y / r };
    }
}

struct SymWg; // stream_blocks.hip: a workgroup's entry of the symbol filter's plan (gr4pm_rotator::mc_wg)

} // namespace
} // namespace gr4pm

struct gr4pm_rotator : gr4pm::hostlogic::RotHostState { // mode, delay, n_channels and what the tags carry: hostlogic/rotator_plan.hpp
    float phase_incr;
    hipStream_t stream;
    // [kStates][n_channels], st_cur selects the row a call reads; it writes the next one (round 6: a ring instead of two
    // halves -- the chain kernels of several plans are in flight at once, see PlanSync)
    static constexpr int kStates = GR4PM_CFC_PLANS + 2;
    gr4pm::DevBuf<gr4pm::RotState> state;
    int st_cur = 0;
    // Round 6: the chains of CONSECUTIVE ring plans run side by side.  A plan's segments that start at a set_freq event
    // (or are fixed points) depend on nothing before them: their kernel goes to one of kAux streams of the handle's own.
    // The segments that continue the carried phasor -- at most one per channel -- need the state the plan before wrote:
    // their kernel goes to `dep`, one stream for all plans, behind the other kernel of the plan before.  The consumers
    // (the fused symbol filter) wait for the plan's two events on THEIR stream; the stream the plan was made on carries the
    // uploads only, so the pipeline stage that makes the plans no longer waits for a chain.  With one packet per 2^20
    // samples a chain is 2^20 dependent steps (16.7 ms) per 2^28-sample batch: one behind the other they were the
    // receiver's period (15 Gsps); side by side they are its latency.  GR4PM_ROT_SERIAL=1: one kernel on the handle's stream.
    // Three kernels a plan, each on a stream of its own (kAux of each kind, taken in turn): `writer` = the channels' LAST
    // segments where they start at an event (they write the carried state: the plan behind waits for this kernel alone, not
    // for the other 2^20-step chains of the plan), `indep` = the other event-started segments, `dep` = the continuations.
    static constexpr int kAux = 4;
    hipStream_t aux[3 * kAux] = {};
    bool async_ready = false;
    struct PlanSync {
        hipEvent_t up = nullptr, indep = nullptr, writer = nullptr, dep = nullptr;
        bool async = false;
        bool dep_writes_state = false; // a continuation is its channel's last segment (no event in the call)
    } sync[GR4PM_CFC_PLANS];
    int last_async_plan = -1; // the plan whose kernels wrote the state row st_cur (or -1: written on `stream`)
    // When: a ring plan whose longest chain is at least kAsyncMinItems long (2 ms of dependent steps; packets back to back
    // make chains of 26 000 items and gain nothing: 56.6 -> 55 Gsps with three kernels and their events per plan), in a
    // process whose HIP runtime has at least eight hardware queues (GPU_MAX_HW_QUEUES; its default is four, and a chain
    // kernel that shares a queue with another stream's work holds that work back for as long as it lives: with four
    // queues the side-by-side form is SLOWER than one kernel, 14.8 against 18.3 Gsps at one packet per 2^20 samples,
    // with sixteen it is 41.8).  Read at creation: GR4PM_ROT_SERIAL=1 never, GR4PM_ROT_ASYNC=1 always (tests).
    static constexpr size_t kAsyncMinItems = size_t{ 1 } << 17;
    int async_policy = 0; // 0: by chain length and queue count, 1: always, -1: never
    unsigned test_delay_us = 0; // GR4PM_TEST_ROT_DELAY_US: every chain kernel of an asynchronous plan starts that much later
    // the plan of a call (segment table, phasor checkpoints, increments, counters): a ring of
    // GR4PM_CFC_PLANS sets, so that the next calls can be planned while the consumers of earlier
    // plans are still running (gr4pm_cfc_symbol_filter_plan / _run; buffers are allocated on first use)
    struct Plan {
        gr4pm::DevBuf<gr4pm::hostlogic::RotSeg> segs;
        gr4pm::DevBuf<gr4pm::cf> ck, seg_incr;
        gr4pm::DevBuf<unsigned> seg_counter0, order;
        gr4pm::DevBuf<unsigned> const_list; // the mode-2 segments of THIS plan (its own staging buffer: plans are issued ahead)
        unsigned n_segs = 0;
        size_t n_in = 0;
        std::vector<unsigned> seg_first; // [n_channels + 1]: the segments of channel c are [seg_first[c], seg_first[c + 1])
    } plans[GR4PM_CFC_PLANS];
    int plan_cur = 0;
    bool ring_sized = false;
    // gr4pm_cfc_symbol_filter_run_channels: channel table + runs of all channels (one upload), workgroup plan
    gr4pm::DevBuf<unsigned long long> mc_tab;
    gr4pm::DevBuf<gr4pm::SymWg> mc_wg;
    std::vector<unsigned long long> mc_host;
    // the streams and events are made on first use (rotator_plan); here is the one place they are released
    ~gr4pm_rotator()
    {
        for (auto& y : sync)
            for (hipEvent_t e : { y.up, y.indep, y.writer, y.dep })
                if (e) (void)hipEventDestroy(e);
        for (hipStream_t a : aux)
            if (a) (void)hipStreamDestroy(a);
    }
};

namespace gr4pm {
// rotator.hip: host replay of the tag-driven control flow + the serial phasor checkpoints of one call (see there)
gr4pm_status rotator_plan(::gr4pm_rotator* h, size_t n, const gr4pm_tag* tags, const uint32_t* tag_channel, size_t n_tags,
                          hostlogic::RotPlan& rp, bool ring = false);
// rotator.hip: what reads a ring plan's checkpoints waits for its chains on its own stream
gr4pm_status cfc_wait_plan(::gr4pm_rotator* cfc, int plan, hipStream_t consumer);
} // namespace gr4pm
