"""The host logic of the StreamRowResampler as a stand-alone program under UndefinedBehaviorSanitizer and AddressSanitizer:
tests/hostlogic/row_stream_plan_check.cpp sweeps csrc/hostlogic/row_stream_plan.hpp over Q in {2, 32, 256} x P in {1, 12, 128}
x six steps from 2^26 to 2^38 x start_index in {0, 1, 2^32 - 1, 2^33 + 20480, 2^63} x three phase0 x a dozen cuttings of a
row into calls (lengths 0, 1, P - 2, P - 1, P among them), with and without a set_row in the middle, against the unbounded
definition in __int128: the counts of a cutting sum to one call's, every item's position and theta are the definition's,
the positions the kernel is handed never wrap and never precede ref, set_row keeps p* and the phase there, and no refusal
touches the state.  And the fresh row (start_index 0) over P in {1, 2, 12, 2048} x eight steps from 2^26 to 2^38 x six phase0
up to 2^63 - 1 x n in {0, 1, P - 1, P, 2^32 - P} x the int32 edge words and random ones: d = phase0, ref_frac = 0, the carried
theta is the one-shot's row_theta at the first, the last and random positions below (n + P - 1) 2^32, and the one-shot's count
is the stream's over n + P - 1 items for n > 0 and 0 for n = 0: the two kernels are one body.  No GPU, no HIP, nothing loaded into python."""
import re

from test_carrier_find_check import run_check


def test_row_stream_plan_sweep_under_sanitizers(tmp_path):
    out = run_check(tmp_path, "row_stream_plan_check")
    m = re.fullmatch(r"row_stream_plan_check: (\d+) cases, 0 failures\n", out)
    assert m, out[-2000:]
    assert int(m.group(1)) >= 8 * 6 * 5 * 12
