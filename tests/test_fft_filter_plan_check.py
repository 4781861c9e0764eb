"""The host logic of the FftFilter as a stand-alone program under UndefinedBehaviorSanitizer and AddressSanitizer:
tests/hostlogic/fft_filter_plan_check.cpp sweeps csrc/hostlogic/fft_filter_plan.hpp against restatements in __int128 from
"segment s is the N items from s hop - V" alone: every refusal of the validation (each must occur), the default overlap of
every L, a non-finite tap at every place, and for V in {0, 1, 63, 64, 256, 1024, 1983, 1984} the segments, carried samples,
first output index, reads and flush of call sequences (0 and 1 sample, around hop and around N, single samples across a
segment end, 2^40 samples, 200 random calls).  No GPU, no HIP, nothing loaded into python."""
import re

from test_carrier_find_check import run_check


def test_fft_filter_plan_sweep_under_sanitizers(tmp_path):
    out = run_check(tmp_path, "fft_filter_plan_check")
    m = re.fullmatch(r"fft_filter_plan_check: (\d+) cases, 0 failures\n", out)
    assert m, out[-2000:]
    # the validation's grid, the default overlaps, the taps, and per V four sequences of 9, 9, 12 and 4 calls and 200 random
    assert int(m.group(1)) >= 13 * 13 + 1985 + 1 + 7 * 2 * 3 + 8 * (9 + 9 + 12 + 4 + 200)
