"""The host logic of the RowResampler as a stand-alone program under UndefinedBehaviorSanitizer and AddressSanitizer:
tests/hostlogic/row_resample_plan_check.cpp sweeps csrc/hostlogic/row_resample_plan.hpp over Q in {2, 32, 256} x P in {1, 12,
128} x six steps from 2^26 to 2^38 x row lengths from 0 to 2^32 - P x phase0 up to 2^63 - 1, restated in __int128: a row's
output length, the tile and its span within the stage, the stage's index test, positions that do not wrap, theta, and
every refusal.  No GPU, no HIP, nothing loaded into python."""
import re

from test_carrier_find_check import run_check


def test_row_resample_plan_sweep_under_sanitizers(tmp_path):
    out = run_check(tmp_path, "row_resample_plan_check")
    m = re.fullmatch(r"row_resample_plan_check: (\d+) cases, 0 failures\n", out)
    assert m, out[-2000:]
    assert int(m.group(1)) >= 8 * 6 * 7 * 4 * 3
