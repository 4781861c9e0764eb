"""The host logic of the FftDuc as a stand-alone program under UndefinedBehaviorSanitizer and AddressSanitizer:
tests/hostlogic/fft_duc_plan_check.cpp sweeps csrc/hostlogic/fft_duc_plan.hpp against restatements in __int128 from
a_s = s hop - V alone: every refusal of the validation (each must occur), and for I in {4, 8, 16, 32, 64} x eight overlaps
from 0 to 1984 x three start indices the segments, carried items, samples and segment positions of call sequences (0 and 1
item, around hopI and around B, single items across a segment end, 2^40 items, 200 random calls).  No GPU, no HIP, nothing
loaded into python."""
import re

from test_carrier_find_check import run_check


def test_fft_duc_plan_sweep_under_sanitizers(tmp_path):
    out = run_check(tmp_path, "fft_duc_plan_check")
    m = re.fullmatch(r"fft_duc_plan_check: (\d+) cases, 0 failures\n", out)
    assert m, out[-2000:]
    # the validation's grid, the default overlaps, and per (I, V) four sequences of 9, 9, 12 and 4 calls from three starts
    # and 200 random calls
    assert int(m.group(1)) >= 4 * 8 * 7 * 7 * 11 + 9 + 5 * 8 * (3 * (9 + 9 + 12 + 4) + 200)
