"""The host logic of the MixedFftDuc as a stand-alone program under UndefinedBehaviorSanitizer and AddressSanitizer:
tests/hostlogic/fft_duc_mixed_plan_check.cpp sweeps csrc/hostlogic/fft_duc_mixed_plan.hpp against restatements in __int128
from a_s = s hop - V and "item m of row k sits at output sample m I_k" alone: every refusal of the validation (each must
occur, the one for a single row included), and for all 31 non-empty subsets of {4, 8, 16, 32, 64} x seven overlaps from 0
to 1984 x three start indices the segments, the items taken, carried and left per row (taken = delivered + carried,
H_k < B_k), the samples and the segment positions of call sequences in slots (0 and 1 slot, around hop / Imax and around
N / Imax, single slots across a segment end, 2^40 items in the longest row, 200 random calls).  No GPU, no HIP, nothing
loaded into python."""
import re

from test_carrier_find_check import run_check


def test_fft_duc_mixed_plan_sweep_under_sanitizers(tmp_path):
    out = run_check(tmp_path, "fft_duc_mixed_plan_check")
    m = re.fullmatch(r"fft_duc_mixed_plan_check: (\d+) cases, 0 failures\n", out)
    assert m, out[-2000:]
    # the validation's grid, the row-specific refusal, the default overlaps, and per (subset, V) four sequences of 9, 9, 12
    # and 4 calls from three starts and 200 random calls
    assert int(m.group(1)) >= 5 * 6 * 6 * 5 * 2 * 11 + 1 + 27 + 31 * 7 * (3 * (9 + 9 + 12 + 4) + 200)
