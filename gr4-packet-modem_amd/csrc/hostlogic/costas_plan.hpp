// hostlogic/costas_plan.hpp -- CostasLoop (costas_loop.hpp:52-148) without HIP: the loop coefficients of
// settingsChanged() and the tag-driven half of a call.  The PLL is serial, but a syncword_phase tag resets its state
// completely (:35-42, :101-106), so the items between two such tags are independent of everything before them: the host
// cuts the call there and the kernels run one lane per segment (process / process_ragged) or per chain of pieces
// (process_packets: the settings follow the packet tags, phase and frequency flow from piece to piece).
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "base.hpp"

namespace gr4pm {
namespace hostlogic {

struct CostasSeg {
    unsigned long long start;
    unsigned len;
    unsigned channel;
    int mode; // 0 continue, 1 set_phase(phase0)
    int last;
    float phase0;
    float pad;
};
static_assert(sizeof(CostasSeg) == 32, "the kernels' record");
// Tag-driven settings (gr4pm_costas_loop_process_packets): a chain is the run of items between
// two set_phase events; it consists of pieces with their own constellation and loop
// coefficients (syncword: PILOT, header and payload: QPSK with different bandwidths); phase
// and frequency flow from piece to piece.  One lane per chain.
struct CostasPiece {
    unsigned long long start; // first item of the piece in the loop's OUTPUT (= its input stream's index)
    long long in_off;         // its input items are in[start + in_off ...]: 0, or the gather of the block in front folded in
    unsigned len;
    int constellation;
    float k1, k2;
    unsigned pad;
};
static_assert(sizeof(CostasPiece) == 40, "the kernels' record");
struct CostasChain {
    unsigned piece0, n_pieces;
    int mode; // 0 continue from the carried state, 1 set_phase(phase0)
    int last;
    float phase0;
    unsigned pad;
};
static_assert(sizeof(CostasChain) == 24, "the kernels' record");

struct CostasHostState {
    double loop_bandwidth = 0.0;
    int constellation = 0; // 0 PILOT, 1 BPSK, 2 QPSK
    float k1 = 0.0f, k2 = 0.0f;
    struct Memo {
        bool valid = false;
        double bw = 0.0;
        int constellation = 0;
        float k1 = 0.0f, k2 = 0.0f;
    } memo[4];
    unsigned memo_next = 0;
};

inline void costas_coeffs(CostasHostState& h)
{
    // tag-driven settings alternate between a handful of (bandwidth, constellation) pairs, three
    // times per packet: remember the last few results instead of redoing the cube roots
    for (const auto& m : h.memo)
        if (m.valid && m.bw == h.loop_bandwidth && m.constellation == h.constellation) {
            h.k1 = m.k1;
            h.k2 = m.k2;
            return;
        }
    // settingsChanged(), costas_loop.hpp:62-87
    double gain = 1.0;
    if (h.constellation == 2) gain = 1.41421356237309504880;
    const double bw = h.loop_bandwidth, bw2 = bw * bw, bw3 = bw2 * bw, bw4 = bw2 * bw2;
    const double s = std::cbrt(36.0 * bw2 +
                               std::sqrt(3.0) * std::sqrt(432.0 * bw4 + 848.0 * bw3 + 624.0 * bw2 +
                                                          204.0 * bw + 25.0) +
                               36.0 * bw + 9.0);
    const double z = -(-12.0 * bw - 6.0) / (3.0 * std::cbrt(6.0) * (2.0 * bw + 1.0) * s) +
                     (std::cbrt(2.0) * s) / (std::cbrt(9.0) * (2.0 * bw + 1.0)) - 1.0;
    h.k1 = static_cast<float>((1.0 - z * z) / gain);
    h.k2 = static_cast<float>(((1.0 - z) * (1.0 - z)) / gain);
    auto& slot = h.memo[h.memo_next++ % 4];
    slot = { true, h.loop_bandwidth, h.constellation, h.k1, h.k2 };
}

// process / process_ragged.  n_of(c): items of channel c in this call (channels with 0 items keep their state)
template <typename NOf>
inline void costas_segments(size_t n_channels, NOf n_of, const gr4pm_tag* tags, const uint32_t* tag_channel, size_t n_tags,
                            bool no_sort, std::vector<CostasSeg>& segs)
{
    for (size_t c = 0; c < n_channels; ++c) {
        const size_t n = n_of(c);
        if (n == 0) { // a piece of length 0 that only hands the carried state on to the other slot
            CostasSeg g{};
            g.channel = static_cast<unsigned>(c);
            g.last = 1;
            segs.push_back(g);
            continue;
        }
        size_t pos = 0;
        int mode = 0;
        float phase0 = 0.0f;
        auto push = [&](size_t end) {
            if (end <= pos) return;
            CostasSeg g{};
            g.start = pos;
            g.len = static_cast<unsigned>(end - pos);
            g.channel = static_cast<unsigned>(c);
            g.mode = mode;
            g.phase0 = phase0;
            g.last = 0;
            segs.push_back(g);
            pos = end;
        };
        for (size_t t = 0; t < n_tags; ++t) {
            const size_t tc = tag_channel ? tag_channel[t] : 0;
            if (tc != c || !(tags[t].flags & GR4PM_TAG_SYNCWORD) || tags[t].index >= n) continue;
            const size_t i = static_cast<size_t>(tags[t].index);
            push(i);
            if (i == pos) { // set_phase at the head of the chunk, costas_loop.hpp:101-106
                mode = 1;
                phase0 = tags[t].phase;
            }
        }
        push(n);
        if (!segs.empty() && segs.back().channel == c) segs.back().last = 1;
    }
    // A wave lives as long as its longest lane.  Segments are independent of one another (carried state travels through
    // the ping-pong state array, not through their order), so the longest ones are put together: a stream with missed
    // detections (segments that run through several packets: 64 channels of configs[2] hold ~80 of five packets'
    // length among 9700) then keeps two waves alive for the long tail instead of eighty.
    if (!no_sort)
        std::stable_sort(segs.begin(), segs.end(), [](const CostasSeg& a, const CostasSeg& b) { return a.len > b.len; });
}

// process_packets over a single-channel loop.  The loop's input stream need not be in memory as such: item i of it is
// `in[spans[k].src + (i - spans[k].dst)]` for the span that holds i (ascending, covering [0, n)); spans == nullptr: the
// stream is `in` itself.  The settings FOLLOW THE TAGS as the table is made -- h is advanced in place, tag by tag -- and a
// refused call (a constellation above 2, a span table with a hole) leaves the settings of the tags in front of the
// refusal applied: the caller has no earlier state to return to, and the reference's block has none either.
inline gr4pm_status costas_packet_chains(CostasHostState& h, const CopySpan* spans, size_t n_spans, size_t n,
                                         const gr4pm_packet_tag* tags, size_t n_tags, std::vector<CostasChain>& chains,
                                         std::vector<CostasPiece>& pieces)
{
    CostasChain cur{};
    cur.piece0 = 0;
    cur.mode = 0;
    size_t pos = 0;
    size_t span_at = 0; // cursor into spans (pieces are closed in ascending order)
    auto close_piece = [&](size_t end) {
        while (pos < end) {
            size_t stop = end;
            long long in_off = 0;
            if (spans) {
                while (span_at < n_spans && spans[span_at].dst + spans[span_at].len <= pos) ++span_at;
                if (span_at >= n_spans || spans[span_at].dst > pos) { // (a hole in the table: the caller's error)
                    pos = end;
                    span_at = n_spans + 1;
                    return;
                }
                stop = std::min<size_t>(end, spans[span_at].dst + spans[span_at].len);
                in_off = static_cast<long long>(spans[span_at].src) - static_cast<long long>(spans[span_at].dst);
            }
            while (pos < stop) { // (len is 32 bits wide)
                const size_t m = std::min<size_t>(stop - pos, 1u << 30);
                CostasPiece pc{};
                pc.start = pos;
                pc.in_off = in_off;
                pc.len = static_cast<unsigned>(m);
                pc.constellation = h.constellation;
                pc.k1 = h.k1;
                pc.k2 = h.k2;
                pieces.push_back(pc);
                pos += m;
            }
        }
    };
    auto close_chain = [&]() {
        cur.n_pieces = static_cast<unsigned>(pieces.size()) - cur.piece0;
        if (cur.n_pieces) chains.push_back(cur);
        cur = CostasChain{};
        cur.piece0 = static_cast<unsigned>(pieces.size());
    };
    for (size_t t = 0; t < n_tags; ++t) {
        if (tags[t].index >= n) break;
        close_piece(static_cast<size_t>(tags[t].index));
        // keys naming settings are applied before the chunk, then settingsChanged(), :52-88
        bool changed = false;
        if (tags[t].constellation >= 0) {
            if (tags[t].constellation > 2) {
                set_error("constellation %d", tags[t].constellation);
                return GR4PM_ERR_INVALID;
            }
            h.constellation = tags[t].constellation;
            changed = true;
        }
        if (tags[t].loop_bandwidth >= 0.0) {
            h.loop_bandwidth = tags[t].loop_bandwidth;
            changed = true;
        }
        if (changed) costas_coeffs(h);
        if (tags[t].kind == GR4PM_PKT_SYNCWORD && (tags[t].syncword.flags & GR4PM_TAG_SYNCWORD)) { // :101-106
            close_chain();
            cur.mode = 1;
            cur.phase0 = tags[t].syncword.phase;
        }
    }
    close_piece(n);
    close_chain();
    if (span_at > n_spans) {
        set_error("process_packets: the span table does not cover the stream");
        return GR4PM_ERR_INVALID;
    }
    if (!chains.empty()) chains.back().last = 1;
    return GR4PM_OK;
}

} // namespace hostlogic
} // namespace gr4pm
