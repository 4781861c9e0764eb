"""The host logic of the Spectrogram block as stand-alone programs under UndefinedBehaviorSanitizer and AddressSanitizer:
tests/hostlogic/spectrogram_plan_check.cpp sweeps csrc/hostlogic/spectrogram_plan.hpp (rows, carry and the hand-out of
rows to waves of every call) over every hop and R in {1, 2, 3, 64}, tests/hostlogic/burst_find_check.cpp runs
csrc/hostlogic/burst_find.hpp on synthetic power series with room for all bursts, for one and for none.  No GPU, no HIP,
nothing loaded into python."""
import re

from test_carrier_find_check import run_check


def test_spectrogram_plan_sweep_under_sanitizers(tmp_path):
    """every hop in 1 .. 2048 x R in {1, 2, 3, 64}, calls of 0, 1, hop - 1, hop, N - 1, N, N + 1 and 3 N + 7 samples in
    four orders: the rows of the calls sum to segments(T) / R, carry_out of a call is carry_in of the next, every row is
    assigned to exactly one wave, and no segment reads outside the tail plus the input"""
    out = run_check(tmp_path, "spectrogram_plan_check")
    m = re.fullmatch(r"spectrogram_plan_check: (\d+) calls, 0 failures\n", out)
    assert m, out[-2000:]
    assert int(m.group(1)) == 2048 * 4 * 4 * 16


def test_burst_find_under_sanitizers(tmp_path):
    out = run_check(tmp_path, "burst_find_check")
    m = re.fullmatch(r"burst_find_check: (\d+) cases, 0 failures\n", out)
    assert m, out[-2000:]
    assert int(m.group(1)) >= 19
