// Sweeps csrc/hostlogic/row_gate_plan.hpp (the RowBurstGate's host side) against a restatement that
// sees all block sums of a row at once: the records of every cutting of a row into calls, and of the flush behind it, are
// the restatement's, field by field; every span lies inside what the device retained before the call and inside the items
// that exist; the retained items stay inside their bound; a call planned with a capacity below its count leaves the rows
// as they were and the same call with the count goes through; and the refusals of the parameters and of a call's arrays.
// Stand-alone, built with -fsanitize=undefined,address by tests/test_row_gate_plan_check.py.
//
// Block sums take three levels, 1, 3 and 5, against close_sum 2 and open_sum 4: below close, between, above open.  A
// set_thresholds in the middle moves them to 0.5 and 2.5 (then 1 lies between and 3 above open), or to 4 and 6 (then
// nothing opens).  Parameters: hold 0 .. 3, min 1 .. 3, pre 0 .. 3, post 0 .. hold + 1, max_blocks from pre + min + post
// to 12: 1000 and more sets.  Sequences of up to 4 blocks meet every set; those of 5 .. 12 blocks (all 3^n of each length)
// take the sets in turn, so every set meets hundreds of them; two random sequences of up to 400 blocks meet every set.
// Each (sequence, set) is run in twelve cuttings, calls of 0 items among them, with and without a partial block at the end.
#include "hostlogic/row_gate_plan.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace gr4pm::hostlogic;

static unsigned long long cases = 0, failures = 0;

#define CHECK(cond, ...)                                                                                                    \
    do {                                                                                                                    \
        if (!(cond)) {                                                                                                      \
            if (++failures <= 20) {                                                                                         \
                std::printf("FAILED %s (line %d): ", #cond, __LINE__);                                                      \
                std::printf(__VA_ARGS__);                                                                                   \
                std::printf("\n");                                                                                          \
            }                                                                                                               \
        }                                                                                                                   \
    } while (0)

static const uint32_t kB = 16;
static const float kLevel[3] = {1.0f, 3.0f, 5.0f};

struct Rec {
    uint64_t first_item, n_items, first_active_item, active_items;
    uint32_t flags;
    float peak;
    double power;
};

static bool same(const Rec& a, const Rec& b)
{
    return a.first_item == b.first_item && a.n_items == b.n_items && a.first_active_item == b.first_active_item &&
           a.active_items == b.active_items && a.flags == b.flags && a.peak == b.peak && a.power == b.power;
}

// the whole row at once: sums of its nb blocks (the last one zero-completed when the row has a partial block), the
// thresholds each block is decided against, n_items items in all; then the flush
static void restate(const std::vector<float>& s, const std::vector<float>& opens, const std::vector<float>& closes, uint64_t n_items,
                    const RowGateParams& p, std::vector<Rec>& out, uint64_t& dropped, uint64_t& truncated)
{
    const size_t nb = s.size();
    out.clear(), dropped = truncated = 0;
    size_t b = 0;
    while (b < nb) {
        if (!(s[b] >= opens[b])) {
            ++b;
            continue;
        }
        const size_t fa = b, start = b > p.pre ? b - p.pre : 0;
        size_t la = b, c = b, run = 0, end = 0;
        uint32_t flags = 0;
        bool done = false;
        for (;; ++c) {
            if (c == nb) break;
            if (c > fa) {
                if (s[c] >= closes[c]) {
                    la = c, run = 0;
                } else if (++run == size_t(p.hold) + 1) {
                    end = la + p.post, done = true;
                    break;
                }
            }
            if (c - start + 1 == p.max_blocks) {
                end = c, flags = kRowGateTruncated, done = true;
                break;
            }
        }
        if (!done) end = la + p.post < nb - 1 ? la + p.post : nb - 1, flags = kRowGateAtEnd;
        if (flags != kRowGateTruncated && la - fa + 1 < p.min_blocks) {
            ++dropped;
        } else {
            Rec r = {};
            double acc = 0.0;
            float peak = s[fa];
            for (size_t i = fa; i <= la; ++i)
                if (i == fa || s[i] >= closes[i]) {
                    acc += static_cast<double>(s[i]);
                    if (s[i] > peak) peak = s[i];
                }
            const uint64_t last = (end + 1) * uint64_t(kB) < n_items ? (end + 1) * uint64_t(kB) : n_items;
            const uint64_t alast = (la + 1) * uint64_t(kB) < n_items ? (la + 1) * uint64_t(kB) : n_items;
            r.first_item = start * uint64_t(kB), r.n_items = last - r.first_item;
            r.first_active_item = fa * uint64_t(kB), r.active_items = alast - r.first_active_item;
            r.flags = flags, r.peak = peak, r.power = acc / static_cast<double>(r.active_items);
            if (flags & kRowGateTruncated) ++truncated;
            out.push_back(r);
        }
        b = done ? c + 1 : nb;
    }
}

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

// the k-th cutting of N items into calls
static const std::vector<uint64_t>& cutting(unsigned k, uint64_t N)
{
    static std::vector<uint64_t> cut; // (kept between the runs, as the vectors of run_row are: the sweep is millions of runs)
    cut.clear();
    uint32_t seed = 977u * k + 1u;
    uint64_t left = N;
    auto take = [&](uint64_t n) {
        n = n < left ? n : left;
        cut.push_back(n);
        left -= n;
    };
    if (k == 0) take(N);
    if (k == 2) take(0);
    while (left != 0) {
        switch (k) {
        case 1: take(kB); break;
        case 2: take(N); break;
        case 3: take(kB - 1); break;
        case 4: take(kB + 1); break;
        case 5: take(2 * kB), take(0); break;
        case 6: take(kB / 2); break;
        case 7: take(3 * kB - 1); break;
        default: take(lcg(seed) >> 16 & 1 ? (lcg(seed) >> 20) % (3 * kB + 1) : 0); break;
        }
    }
    if (k == 5 || k > 7) take(0);
    return cut;
}

// one row through the plan in the given cutting; mode: 0 no set_thresholds, 1: to (2.5, 0.5) in the middle, 2: to (6, 4)
static void run_row(const std::vector<float>& sums, uint64_t tail, const RowGateParams& p, unsigned k, int mode)
{
    ++cases;
    const size_t full = sums.size() - (tail ? 1 : 0);
    const uint64_t N = full * uint64_t(kB) + tail;
    const std::vector<uint64_t>& cut = cutting(k, N);
    RowGateRow row = {}, next = {};
    row.open_sum = 4.0f, row.close_sum = 2.0f;
    static std::vector<float> opens, closes;
    static std::vector<Rec> got, want;
    static std::vector<RowGateSpan> spans;
    static std::vector<uint32_t> span_row;
    opens.clear(), closes.clear(), got.clear();
    const uint64_t offs[1] = {0};
    uint64_t items = 0;
    auto call = [&](uint64_t n, bool flush) {
        const uint64_t before = items / kB;
        if (!flush) items += n;
        const uint64_t after = flush ? sums.size() : items / kB;
        CHECK(flush || row_gate_blocks_for(row, kB, n) == after - before, "blocks of a call");
        for (uint64_t b = before; b < after; ++b) opens.push_back(row.open_sum), closes.push_back(row.close_sum);
        const uint32_t nb[1] = {static_cast<uint32_t>(after - before)};
        const uint64_t len[1] = {n};
        const float* s = sums.data() + before; // (one past the end when the call decides nothing: not read)
        const RowGateRow snapshot = row;
        // room for a span per block and one for the row's end: no call emits more
        spans.assign(nb[0] + 1, RowGateSpan{}), span_row.assign(nb[0] + 1, 99u);
        const size_t count = row_gate_plan_call(&row, &next, 1, p, s, offs, nb, len, flush, spans.data(), span_row.data(), nb[0] + 1);
        CHECK(count <= nb[0] + 1, "%zu spans from %u blocks", count, nb[0]);
        CHECK(std::memcmp(&snapshot, &row, sizeof row) == 0, "planning moved the row");
        if (count >= 1) { // a capacity one below the count: the first spans only, inside their array, and the row stays;
                          // then the same call again with the count
            spans.assign(count - 1, RowGateSpan{}), span_row.assign(count - 1, 99u);
            const size_t again = row_gate_plan_call(&row, &next, 1, p, s, offs, nb, len, flush, spans.data(), span_row.data(), count - 1);
            CHECK(again == count, "the count under a small capacity: %zu, %zu", again, count);
            CHECK(std::memcmp(&snapshot, &row, sizeof row) == 0, "a capacity refusal moved the row");
            spans.assign(count, RowGateSpan{}), span_row.assign(count, 99u);
            const size_t final_count = row_gate_plan_call(&row, &next, 1, p, s, offs, nb, len, flush, spans.data(), span_row.data(), count);
            CHECK(final_count == count, "the count of the same call again");
        }
        for (size_t i = 0; i < count; ++i) {
            const RowGateRecord r = row_gate_record(spans[i], kB, next.items);
            CHECK(span_row[i] == 0, "the span's row");
            CHECK(spans[i].start >= row.keep_first, "a span in front of what the device retains");
            CHECK(r.first_item + r.n_items <= next.items && r.n_items >= 1, "a span behind the row's items");
            CHECK(spans[i].end - spans[i].start + 1 <= p.max_blocks, "a span of more than max_blocks");
            got.push_back(Rec{r.first_item, r.n_items, r.first_active_item, r.active_items, r.flags, r.peak, r.power});
        }
        row = next; // commit
        CHECK(row.items == items, "the item count");
        if (!flush) {
            CHECK(row.decided == items / kB, "the blocks decided");
            CHECK(row_gate_retained(row, kB) <= row_gate_retained_bound(p), "retains %llu items",
                  static_cast<unsigned long long>(row_gate_retained(row, kB)));
            CHECK(row.keep_first >= snapshot.keep_first, "the retained items move backwards");
            CHECK(row.hist == (snapshot.hist ^ (n != 0 ? 1u : 0u)), "the buffer flips with new items only");
        }
    };
    for (size_t i = 0; i < cut.size(); ++i) {
        if (mode != 0 && i == cut.size() / 2) {
            if (mode == 1) row.open_sum = 2.5f, row.close_sum = 0.5f;
            if (mode == 2) row.open_sum = 6.0f, row.close_sum = 4.0f;
        }
        call(cut[i], false);
    }
    call(0, true);
    uint64_t dropped = 0, truncated = 0;
    restate(sums, opens, closes, N, p, want, dropped, truncated);
    CHECK(got.size() == want.size(), "%zu records, the restatement has %zu (cutting %u, %zu blocks)", got.size(), want.size(), k, sums.size());
    for (size_t i = 0; i < got.size() && i < want.size(); ++i)
        CHECK(same(got[i], want[i]), "record %zu: first %llu n %llu flags %u, want first %llu n %llu flags %u", i,
              static_cast<unsigned long long>(got[i].first_item), static_cast<unsigned long long>(got[i].n_items), got[i].flags,
              static_cast<unsigned long long>(want[i].first_item), static_cast<unsigned long long>(want[i].n_items), want[i].flags);
    CHECK(row.emitted == want.size() && row.dropped == dropped && row.truncated == truncated, "the counters");
}

static void refusals()
{
    ++cases;
    const RowGateParams ok = {64, 3, 2, 4, 4, 64};
    CHECK(row_gate_params_check(64, ok, 4096) == RowGateRefusal::none, "the defaults");
    CHECK(row_gate_params_check(65, ok, 4096) == RowGateRefusal::rows && row_gate_params_check(0, ok, 4096) == RowGateRefusal::rows, "rows");
    for (uint32_t B : {0u, 8u, 48u, 100u, 2048u}) {
        RowGateParams p = ok;
        p.B = B;
        CHECK(row_gate_params_check(1, p, 1 << 20) == RowGateRefusal::block, "block %u", B);
    }
    for (uint32_t B : {16u, 32u, 64u, 128u, 256u, 512u, 1024u}) {
        RowGateParams p = ok;
        p.B = B;
        CHECK(row_gate_params_check(1, p, uint64_t(64) * B) == RowGateRefusal::none, "block %u", B);
        CHECK(row_gate_params_check(1, p, uint64_t(64) * B - 1) == RowGateRefusal::columns, "columns of block %u", B);
    }
    RowGateParams p = ok;
    p.post = 5;
    CHECK(row_gate_params_check(1, p, 4096) == RowGateRefusal::post, "post");
    p = ok, p.min_blocks = 0;
    CHECK(row_gate_params_check(1, p, 4096) == RowGateRefusal::min_blocks, "min");
    p = ok, p.max_blocks = 9;
    CHECK(row_gate_params_check(1, p, 4096) == RowGateRefusal::budget, "budget");
    p = ok, p.max_blocks = 10;
    CHECK(row_gate_params_check(1, p, 4096) == RowGateRefusal::none, "budget met");
    p = ok, p.pre = p.min_blocks = 0xffffffffu, p.hold = 0x7fffffffu, p.post = 0x80000000u, p.max_blocks = 0xffffffffu;
    CHECK(row_gate_params_check(1, p, 4096) == RowGateRefusal::budget, "a budget beyond 32 bits");
    p = ok, p.hold = 0x80000000u;
    CHECK(row_gate_params_check(1, p, 4096) == RowGateRefusal::hold, "hold");
    CHECK(row_gate_params_check(1, ok, (uint64_t(1) << 30) + 1) == RowGateRefusal::columns, "columns beyond 2^30");
    CHECK(!row_gate_thresholds_valid(1.0f, 2.0f) && !row_gate_thresholds_valid(1.0f, 0.0f) && row_gate_thresholds_valid(1.0f, 1.0f),
          "thresholds");
    size_t at = 0;
    uint64_t len[2] = {10, 20};
    CHECK(row_gate_call_check(ok, 2, true, 20, len, true, true, true, 4, &at) == RowGateRefusal::none, "a call");
    CHECK(row_gate_call_check(ok, 2, true, 19, len, true, true, true, 4, &at) == RowGateRefusal::length && at == 1, "length");
    CHECK(row_gate_call_check(ok, 2, false, 20, len, true, true, true, 4, &at) == RowGateRefusal::pointer, "no x");
    CHECK(row_gate_call_check(ok, 2, true, 20, nullptr, true, true, true, 4, &at) == RowGateRefusal::pointer, "no lengths");
    CHECK(row_gate_call_check(ok, 2, true, 20, len, false, true, true, 4, &at) == RowGateRefusal::pointer, "no out");
    CHECK(row_gate_call_check(ok, 2, true, 20, len, false, false, true, 0, &at) == RowGateRefusal::none, "no out, no room");
    CHECK(row_gate_call_check(ok, 2, true, 20, len, true, true, false, 4, &at) == RowGateRefusal::pointer, "no count");
    len[0] = (uint64_t(1) << 32) - 4096;
    CHECK(row_gate_call_check(ok, 2, true, uint64_t(1) << 33, len, true, true, true, 4, &at) == RowGateRefusal::items && at == 0, "items");
    len[0] -= 1;
    CHECK(row_gate_call_check(ok, 2, true, uint64_t(1) << 33, len, true, true, true, 4, &at) == RowGateRefusal::none, "items below");
    len[0] = len[1] = 0;
    CHECK(row_gate_call_check(ok, 2, false, 0, len, true, true, true, 4, &at) == RowGateRefusal::none, "nothing to read");
}

int main()
{
    refusals();
    std::vector<RowGateParams> sets;
    for (uint32_t hold = 0; hold <= 3; ++hold)
        for (uint32_t mn = 1; mn <= 3; ++mn)
            for (uint32_t pre = 0; pre <= 3; ++pre)
                for (uint32_t post = 0; post <= hold + 1; ++post)
                    for (uint32_t mx = pre + mn + post; mx <= 12; ++mx) sets.push_back(RowGateParams{kB, hold, mn, pre, post, mx});
    std::vector<float> sums;
    size_t turn = 0;
    auto all_cuttings = [&](const RowGateParams& p, unsigned long long id) {
        for (unsigned k = 0; k < 12; ++k) {
            // the last block as a partial one (of 1 + id % 15 items) in every other run; a set_thresholds in every third
            const uint64_t tail = (k + id) % 2 != 0 ? 1 + id % (kB - 1) : 0;
            run_row(sums, tail, p, k, static_cast<int>((k + id / 2) % 3 == 0 ? 1 + (id / 6) % 2 : 0));
        }
    };
    for (size_t n = 1; n <= 12; ++n) {
        size_t total = 1;
        for (size_t i = 0; i < n; ++i) total *= 3;
        for (size_t code = 0; code < total; ++code) {
            sums.resize(n);
            size_t v = code;
            for (size_t i = 0; i < n; ++i, v /= 3) sums[i] = kLevel[v % 3];
            if (n <= 4) {
                for (const RowGateParams& p : sets) all_cuttings(p, code);
            } else {
                all_cuttings(sets[turn++ % sets.size()], code);
            }
        }
    }
    uint32_t seed = 2031;
    for (size_t i = 0; i < sets.size(); ++i)
        for (int rep = 0; rep < 2; ++rep) {
            sums.resize(13 + (lcg(seed) >> 8) % 388);
            // runs of a level, so that long bursts, long silences and forced splits all occur
            for (size_t j = 0; j < sums.size();) {
                const float level = kLevel[(lcg(seed) >> 12) % 3];
                for (size_t run = 1 + (lcg(seed) >> 10) % (rep ? 9 : 3); run != 0 && j < sums.size(); --run) sums[j++] = level;
            }
            all_cuttings(sets[i], i * 2 + rep);
        }
    std::printf("row_gate_plan_check: %llu cases, %llu failures\n", cases, failures);
    return failures ? 1 : 0;
}
