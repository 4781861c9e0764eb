"""The host logic of the MixedFftDdc as a stand-alone program under UndefinedBehaviorSanitizer and AddressSanitizer:
tests/hostlogic/fft_ddc_mixed_plan_check.cpp sweeps csrc/hostlogic/fft_ddc_mixed_plan.hpp against restatements in __int128
from a_s = s hop - V + Dmax - 1 and the Ddc's frame grid alone: every refusal (channels, a decimation, an image count, taps,
overlap multiple, overlap high, and overlap low for the channel whose Dmax - D_k + L_k - 1 exceeds V), the default overlap,
and for the 31 non-empty subsets of {4, 8, 16, 32, 64} as a handle's decimations x the overlaps from 0 to 1984 that suit
them x three start indices the kept items of every channel and the segments, tails and per-channel frames of the call
sequences of fft_ddc_plan_check.cpp.  No GPU, no HIP, nothing loaded into python."""
import re

from test_carrier_find_check import run_check


def test_fft_ddc_mixed_plan_sweep_under_sanitizers(tmp_path):
    out = run_check(tmp_path, "fft_ddc_mixed_plan_check")
    m = re.fullmatch(r"fft_ddc_mixed_plan_check: (\d+) cases, 0 failures\n", out)
    assert m, out[-2000:]
    # the refusals, 2000 default overlaps, and per subset at least four overlaps x (3 x 36 + 200) calls
    assert int(m.group(1)) >= 11 * 8 * 12 * 13 * 2 + 2000 + 31 * 4 * (3 * 36 + 200)
