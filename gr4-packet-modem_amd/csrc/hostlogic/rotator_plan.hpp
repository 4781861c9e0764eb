// hostlogic/rotator_plan.hpp -- Rotator (rotator.hpp:44-65) and CoarseFrequencyCorrection
// (coarse_frequency_correction.hpp:50-98) without HIP: the tag-driven half of a call.  The phasor recurrence is serial
// per segment, so the host replays the set_freq events over the TAG LIST and hands the kernels a segment table
// (RotSeg), the order its serial lanes take the segments in and the list of segments that need no chain at all.
// rot_plan() is a function from (carried host state, call) to (new host state, tables): it touches nothing of the
// handle, which takes the new state over once the uploads and launches of the call have succeeded.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "base.hpp"

namespace gr4pm {
namespace hostlogic {

struct RotSeg {
    unsigned long long start; // offset inside the channel row
    unsigned long long len;
    unsigned channel;
    unsigned ck0;  // first checkpoint slot of this segment
    int mode;      // 0 continue from state[channel]; 1 set_freq: (exp0, incr); 2 fixed point: the constant (exp0, incr)
    int last;      // writes state[channel] back
    cf exp0, incr;
};
static_assert(sizeof(RotSeg) == 48, "the kernels' record");
constexpr unsigned kRotChunk = 8; // samples per checkpoint

// what a call advances, per channel
struct RotCarried {
    std::vector<float> next_freq;      // coarse_frequency_correction.hpp:44
    std::vector<long> next_freq_delay; // :45
    // The carried phasor is a fixed point of the recurrence -- exp = (1, -+0) with incr = (1, -+0): every product
    // e * incr gives e again and the renormalisation divides by hypot(1, 0) = 1.  That is the state of a
    // CoarseFrequencyCorrection from start() to its first syncword_freq tag (set_freq(0) on the first item,
    // coarse_frequency_correction.hpp:44-45,84-86), after every tag whose frequency is exactly 0, and of a Rotator with
    // phase_incr 0: the stream the reference publishes its receiver benchmark on (zeros: no tag, ever) and every
    // stream until its first detection.  Such a segment needs no serial chain: its checkpoints are the constant
    // (k_rot_const_fill, parallel), the consumers multiply by it as before -- the same bits (x * (1, -0) is not a
    // copy: it turns -0 into +0 in places, as the reference's multiplication does).
    std::vector<uint8_t> fixed;
    std::vector<cf> fixed_exp, fixed_incr;
};
struct RotHostState {
    int mode = 0; // 0 Rotator, 1 CoarseFrequencyCorrection
    size_t delay = 0, n_channels = 0;
    RotCarried carried;
};
// start(): (exp, incr) is the phasor state every channel starts from
inline void rot_reset(RotHostState& h, cf exp, cf incr)
{
    h.carried.next_freq.assign(h.n_channels, 0.0f);
    h.carried.next_freq_delay.assign(h.n_channels, 0); // :45 -> set_freq(0) on the first item
    // (a Rotator whose increment is (1, +-0) never leaves exp = (1, +0); a CFC starts with set_freq(0) on item 0)
    h.carried.fixed.assign(h.n_channels, h.mode == 0 && incr.x == 1.0f && incr.y == 0.0f ? 1 : 0);
    h.carried.fixed_exp.assign(h.n_channels, exp);
    h.carried.fixed_incr.assign(h.n_channels, incr);
}

// The plan of one call.  Caller-owned and reused from call to call: the vectors keep their capacity (a batch of the
// receiver has 10 000 segments, and this runs in its plan-making pipeline stage).
struct RotPlan {
    std::vector<RotSeg> segs;        // channel by channel, each channel's by position: they tile its [0, n)
    std::vector<unsigned> seg_first; // [n_channels + 1]: the segments of channel c are [seg_first[c], seg_first[c + 1])
    // order[]: first the segments that depend on nothing before this call (a set_freq event starts them, or they are fixed
    // points), then the ones that continue the carried phasor (mode 0: at most one per channel); each part by descending
    // length, so that the long ones (a stream with missed detections) share waves.  The first part again in two: `indep`,
    // then `writer` = the channels' LAST segments (they write the carried state).
    std::vector<unsigned> order;
    std::vector<unsigned> const_list; // the mode-2 segments
    unsigned n_indep = 0, n_writer = 0;
    bool dep_writes_state = false; // a continuation is its channel's last segment (no event in the call)
    unsigned long long longest_chain = 0, longest_const = 0; // longest segment with / without a serial chain
    unsigned ck_total = 0;                                   // checkpoint slots of the call
    RotCarried carried;                                      // the host state behind this call
    std::vector<unsigned long long> keys;                    // (scratch of the sort)
};

// no_fixed: every segment as a chain (A/B), no_sort: order[] by position inside each part (A/B)
inline void rot_plan(const RotHostState& h, size_t n, const gr4pm_tag* tags, const uint32_t* tag_channel, size_t n_tags,
                     bool no_fixed, bool no_sort, RotPlan& rp)
{
    std::vector<RotSeg>& segs = rp.segs;
    RotCarried& next = rp.carried;
    segs.clear();
    next = h.carried;
    unsigned ck = 0;
    size_t n_const = 0;
    for (size_t c = 0; c < h.n_channels; ++c) {
        // set_freq events (item, freq) of this channel: coarse_frequency_correction.hpp:76-96
        struct Ev {
            size_t at;
            float freq;
        };
        std::vector<Ev> evs;
        bool pending = false;
        size_t pending_at = 0;
        float pending_freq = 0.0f;
        if (h.mode == 1) {
            if (next.next_freq_delay[c] >= 0) {
                pending = true;
                pending_at = static_cast<size_t>(next.next_freq_delay[c]);
                pending_freq = next.next_freq[c];
            }
            for (size_t t = 0; t < n_tags; ++t) {
                const size_t tc = tag_channel ? tag_channel[t] : 0;
                if (tc != c || !(tags[t].flags & GR4PM_TAG_SYNCWORD) || tags[t].index >= n) continue;
                const size_t i = static_cast<size_t>(tags[t].index);
                // a countdown that has not reached zero when the next tag arrives is
                // overwritten (:79-80 runs before the item loop of that chunk)
                if (pending && pending_at < i) evs.push_back({ pending_at, pending_freq });
                pending = true;
                pending_at = i + h.delay;
                pending_freq = static_cast<float>(tags[t].freq); // :79 cast to float
            }
            if (pending && pending_at < n) {
                evs.push_back({ pending_at, pending_freq });
                pending = false;
            }
            next.next_freq[c] = pending_freq;
            next.next_freq_delay[c] = pending ? static_cast<long>(pending_at - n) : -1;
        }
        // pieces of this channel: [0, first event) continues the carried phasor; every event
        // starts a piece with a fresh phasor (set_freq resets _exp and _counter, :55-58)
        size_t pos = 0;
        auto push = [&](size_t start, size_t end, int mode, float freq) {
            if (end <= start) return;
            RotSeg g{};
            g.start = start;
            g.len = end - start;
            g.channel = static_cast<unsigned>(c);
            ck = (ck + 1u) & ~1u; // an even slot: 16-byte checkpoint stores without a test (k_rot_checkpoints_fresh)
            g.ck0 = ck;
            g.mode = mode;
            g.last = 0;
            if (mode == 1) { // set_freq(), :50-59 (float cos/sin of the host libm)
                const float d = static_cast<float>(h.delay);
                g.exp0 = { std::cos(freq * d), -std::sin(freq * d) };
                g.incr = { std::cos(freq), -std::sin(freq) };
                // exp0 = (1, -+0), incr = (1, -+0) (freq = +-0): e * incr == e for ever
                next.fixed[c] = g.exp0.x == 1.0f && g.exp0.y == 0.0f && g.incr.x == 1.0f && g.incr.y == 0.0f;
                next.fixed_exp[c] = g.exp0;
                next.fixed_incr[c] = g.incr;
            }
            if (next.fixed[c] && !no_fixed) { // (mode 0: the carried phasor is the fixed point)
                g.mode = 2;
                g.exp0 = next.fixed_exp[c];
                g.incr = next.fixed_incr[c];
                n_const += 1;
            }
            ck += static_cast<unsigned>((g.len + kRotChunk - 1) / kRotChunk);
            segs.push_back(g);
        };
        for (size_t k = 0; k < evs.size(); ++k) {
            if (evs[k].at > pos) push(pos, evs[k].at, 0, 0.0f); // only possible for k == 0
            const size_t end = k + 1 < evs.size() ? evs[k + 1].at : n;
            push(evs[k].at, end, 1, evs[k].freq);
            pos = end;
        }
        if (pos < n) push(pos, n, 0, 0.0f);
        segs.back().last = 1; // the channel's final piece writes the carried state
    }
    const unsigned n_segs = static_cast<unsigned>(segs.size());
    rp.ck_total = ck; // (slots are handed out in ascending order: the last segment's end)
    rp.seg_first.assign(h.n_channels + 1, n_segs); // segments were generated channel by channel
    for (unsigned i = n_segs; i-- > 0;) rp.seg_first[segs[i].channel] = i;
    for (size_t c = h.n_channels; c-- > 0;) rp.seg_first[c] = std::min(rp.seg_first[c], rp.seg_first[c + 1]);
    rp.n_indep = rp.n_writer = 0;
    rp.dep_writes_state = false;
    {
        // ONE sort over 64-bit keys (part | longest first | position): this runs in the pipeline stage that makes the plans,
        // 10 000 segments a batch -- two stable sorts with indirect comparisons were half a millisecond of that stage
        std::vector<unsigned long long>& keys = rp.keys;
        auto part = [&](unsigned a) { return segs[a].mode == 0 ? 2u : segs[a].last ? 1u : 0u; }; // indep | writer | dep
        keys.resize(n_segs);
        for (unsigned i = 0; i < n_segs; ++i) {
            const unsigned pt = part(i);
            rp.n_indep += pt == 0;
            rp.n_writer += pt == 1;
            rp.dep_writes_state |= pt == 2 && segs[i].last;
            // (a segment is shorter than 2^36 items -- 2^33 checkpoint slots are 32-bit --, a call has fewer than 2^26 segments)
            const unsigned long long by_len = no_sort ? 0ull : (~segs[i].len & ((1ull << 36) - 1));
            keys[i] = (static_cast<unsigned long long>(pt) << 62) | (by_len << 26) | i;
        }
        std::sort(keys.begin(), keys.end());
        rp.order.resize(n_segs);
        for (unsigned i = 0; i < n_segs; ++i) rp.order[i] = static_cast<unsigned>(keys[i] & ((1u << 26) - 1));
    }
    rp.const_list.clear();
    if (n_const)
        for (unsigned i = 0; i < n_segs; ++i)
            if (segs[i].mode == 2) rp.const_list.push_back(i);
    rp.longest_const = rp.longest_chain = 0;
    for (unsigned i = 0; i < n_segs; ++i) {
        unsigned long long& longest = segs[i].mode == 2 ? rp.longest_const : rp.longest_chain;
        longest = std::max(longest, segs[i].len);
    }
}

} // namespace hostlogic
} // namespace gr4pm
