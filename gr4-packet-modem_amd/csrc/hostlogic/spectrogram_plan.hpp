// hostlogic/spectrogram_plan.hpp -- the row and carry arithmetic of the Spectrogram block (spectrogram.hip), HIP-free,
// on top of spectrum_plan.hpp: the segments are exactly the Spectrum's.
//
// Row t is made of the segments t R .. t R + R - 1 of the stream; it exists once segment t R + R - 1 is complete, so
// after S segments there are S / R rows and S mod R segments are summed (or maximised) into the row that is not
// complete yet, the `carry`: 2048 float32 on the device and this count.  A call that completes n_segments segments on
// top of carry_in = S mod R of them sees `units` = ceil((carry_in + n_segments) / R) units: unit u is the call's
// segments
//     [u == 0 ? 0 : u R - carry_in,  min(n_segments, (u + 1) R - carry_in))
// The first `rows` units are complete and become rows u of the call's output; unit 0 starts from the carry iff
// carry_in > 0 (reads_carry), and the unit behind the rows, if there is one, is incomplete and goes to the new carry
// (writes_carry).  A call with no segment has no unit and leaves the carry as it is.
// Units go to waves in runs of `run` consecutive units, as short as `max_waves` waves allow: a wave walks the segments
// of its run back to back, so the run's length only spreads the work.
#pragma once
#include "spectrum_plan.hpp"

namespace gr4pm {
namespace hostlogic {

struct SpectrogramPlan {
    SpectrumPlan seg;   // the call's segments and tail
    size_t carry_in;    // segments in the incomplete row before the call, < R
    size_t rows;        // the call completes these
    size_t carry_out;   // segments in the incomplete row after the call, < R
    size_t units;       // rows, plus one if the call ends inside a row; 0 without a segment
    bool reads_carry;   // unit 0 starts from the carried accumulators
    bool writes_carry;  // unit `rows` exists and writes the new carry
    size_t run;         // units per wave
    size_t waves;       // ceil(units / run) <= max_waves
};

// rows a stream of T samples has made
inline uint64_t spectrogram_rows(uint64_t T, uint64_t N, uint64_t hop, uint64_t R) { return spectrum_segments(T, N, hop) / R; }

// T: samples taken before the call; n: the call's; max_waves >= 1
inline SpectrogramPlan spectrogram_plan(uint64_t T, size_t n, size_t N, size_t hop, size_t R, size_t max_waves)
{
    SpectrogramPlan p;
    p.seg = spectrum_plan(T, n, N, hop);
    p.carry_in = static_cast<size_t>(p.seg.segments_before % R);
    p.rows = (p.carry_in + p.seg.n_segments) / R;
    p.carry_out = static_cast<size_t>((p.seg.segments_before + p.seg.n_segments) % R);
    const bool any = p.seg.n_segments != 0;
    p.units = any ? p.rows + (p.carry_out ? 1 : 0) : 0;
    p.reads_carry = any && p.carry_in != 0;
    p.writes_carry = any && p.carry_out != 0;
    p.run = p.units ? (p.units + max_waves - 1) / max_waves : 1;
    p.waves = (p.units + p.run - 1) / p.run;
    return p;
}

// the call's segments [first, end) of unit u < units
inline size_t spectrogram_unit_first(const SpectrogramPlan& p, size_t R, size_t u) { return u == 0 ? 0 : u * R - p.carry_in; }
inline size_t spectrogram_unit_end(const SpectrogramPlan& p, size_t R, size_t u)
{
    const size_t e = (u + 1) * R - p.carry_in;
    return e < p.seg.n_segments ? e : p.seg.n_segments;
}

} // namespace hostlogic
} // namespace gr4pm
