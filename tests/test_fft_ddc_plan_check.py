"""The host logic of the FftDdc as a stand-alone program under UndefinedBehaviorSanitizer and AddressSanitizer:
tests/hostlogic/fft_ddc_plan_check.cpp sweeps csrc/hostlogic/fft_ddc_plan.hpp against restatements in __int128: the nearest
bin, the rotator's phase and the response table's word for edge and random frequency words, every refusal of the
validation, and for D in {4, 8, 16, 32, 64} x six to eight overlaps from 0 to 1984 x three start indices the segments, tails, frames and segment
positions of call sequences (0 and 1 sample, around a hop and around N, single samples across a segment end, 2^40 samples,
200 random calls).  No GPU, no HIP, nothing loaded into python."""
import re

from test_carrier_find_check import run_check


def test_fft_ddc_plan_sweep_under_sanitizers(tmp_path):
    out = run_check(tmp_path, "fft_ddc_plan_check")
    m = re.fullmatch(r"fft_ddc_plan_check: (\d+) cases, 0 failures\n", out)
    assert m, out[-2000:]
    assert int(m.group(1)) >= 2000 + 4 * 8 * 7 * 7 * 11 + 5 * 6 * (3 * 36 + 200)
