// hostlogic/line_plan.hpp -- the row, segment and run arithmetic of the LineSpectrum block (csrc/line_spectrum.hip,
// DESIGN.md section 23), HIP-free.  The kernels use these constexpr expressions themselves.
//
// A call has R <= 64 rows; row r has n_r items, y[i] = f(gain x[i]) for i < n_r and 0 beyond.  N = 2048, 1 <= hop <= N.
//     segments   S_r = n_r == 0 ? 0 : 1 + ceil(max(n_r - N, 0) / hop); segment s is y[s hop .. s hop + N), zero-filled
//     transforms T_r = S_r, or for the envelope ceil(S_r / 2): transform p takes the segments 2 p and 2 p + 1 as the real
//                and the imaginary part, an odd last segment pairs with zero
//     runs       a wave takes kLineFloatRun = 64 consecutive transforms of one row (the last run of a row: what is left);
//                the run length is fixed, so a row's runs, and with them its bits, depend on that row alone
//     waves      are numbered over the rows in order: row r owns the waves [run_start[r], run_start[r + 1])
// A segment that lies wholly inside [0, n_r) is loaded unguarded; of any other, item i is loaded iff s hop + i < n_r, and a
// segment that does not exist (the zero partner of an odd last one) loads nothing.
#pragma once
#include <cstddef>
#include <cstdint>

namespace gr4pm {
namespace hostlogic {

constexpr uint64_t kLineN = 2048;
constexpr uint64_t kLineFloatRun = 64; // transforms a wave sums in float32
constexpr size_t kLineMaxRows = 64;    // of a call: their lengths and run starts travel by value
constexpr uint64_t kLineMaxItems = uint64_t(1) << 40; // of a row

constexpr uint64_t line_segments(uint64_t n, uint64_t hop)
{
    return n == 0 ? 0 : 1 + (n > kLineN ? (n - kLineN + hop - 1) / hop : 0);
}
constexpr uint64_t line_transforms(uint64_t segments, bool pairs) { return pairs ? (segments + 1) / 2 : segments; }
constexpr uint64_t line_runs(uint64_t transforms) { return (transforms + kLineFloatRun - 1) / kLineFloatRun; }
// transforms of run `run` of a row with `transforms`
constexpr uint64_t line_run_count(uint64_t transforms, uint64_t run)
{
    return transforms - run * kLineFloatRun < kLineFloatRun ? transforms - run * kLineFloatRun : kLineFloatRun;
}
// the items of segment s a row of n items has: the limit a load is guarded by (0: nothing is loaded)
constexpr uint64_t line_segment_limit(uint64_t s, uint64_t segments, uint64_t n) { return s < segments ? n : 0; }
// whether all N items of the segment at item i0 lie below `limit`: the unguarded path
constexpr bool line_unguarded(uint64_t i0, uint64_t limit) { return i0 + kLineN <= limit; }
// whether item i0 + i of a guarded segment is loaded
constexpr bool line_item_loaded(uint64_t i0, uint64_t i, uint64_t limit) { return i0 + i < limit; }

struct LinePlan {
    uint64_t run_start[kLineMaxRows + 1]; // prefix sums of the rows' runs; run_start[R ..] = the total
};

inline LinePlan line_plan(const uint64_t* lengths, size_t R, uint64_t hop, bool pairs)
{
    LinePlan p;
    uint64_t at = 0;
    for (size_t r = 0; r <= kLineMaxRows; ++r) {
        p.run_start[r] = at;
        if (r < R) at += line_runs(line_transforms(line_segments(lengths[r], hop), pairs));
    }
    return p;
}

// the row that owns wave w < run_start[R]: the r with run_start[r] <= w < run_start[r + 1] (rows without runs own no wave)
constexpr uint32_t line_row_of(const uint64_t* run_start, uint32_t R, uint64_t w)
{
    uint32_t r = 0;
    for (uint32_t i = 1; i < R; ++i)
        if (run_start[i] <= w && w < run_start[i + 1]) r = i;
    return r;
}

} // namespace hostlogic
} // namespace gr4pm
