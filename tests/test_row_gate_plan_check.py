"""The host logic of the RowBurstGate as a stand-alone program under UndefinedBehaviorSanitizer and AddressSanitizer:
tests/hostlogic/row_gate_plan_check.cpp sweeps csrc/hostlogic/row_gate_plan.hpp against a restatement that sees all block
sums of a row at once.  Block sums over three levels (below close, between, above open), every sequence of up to 12 blocks
and random ones of up to 400; hold 0 .. 3, min 1 .. 3, pre 0 .. 3, post 0 .. hold + 1, max_blocks from its minimum to 12; a
dozen cuttings each with calls of 0 items; a capacity below the count followed by the same call again; set_thresholds
between calls; flush with and without a partial block.  The records are the restatement's, the retained items stay inside
their bound, every span lies inside what was retained, and no refusal moves the state.  No GPU, no HIP, nothing loaded into
python."""
import re

from test_carrier_find_check import run_check


def test_row_gate_plan_sweep_under_sanitizers(tmp_path):
    out = run_check(tmp_path, "row_gate_plan_check")
    m = re.fullmatch(r"row_gate_plan_check: (\d+) cases, 0 failures\n", out)
    assert m, out[-2000:]
    assert int(m.group(1)) >= 12 * (3 ** 12 + 2 * 1000)
