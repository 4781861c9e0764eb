"""The host logic of the LineSpectrum block as stand-alone programs under UndefinedBehaviorSanitizer and
AddressSanitizer, built and run as tests/test_carrier_find_check.py does: tests/hostlogic/line_plan_check.cpp sweeps
csrc/hostlogic/line_plan.hpp over every hop, line_find_check.cpp runs csrc/hostlogic/line_find.hpp on synthetic spectra
and ratio_check.cpp holds csrc/hostlogic/ratio.hpp against brute force.  No GPU, no HIP, nothing loaded into python."""
import re

from test_carrier_find_check import run_check


def test_line_plan_sweep_under_sanitizers(tmp_path):
    """every hop in 1 .. 2048 x eight lengths x both forms: no index at or beyond a row's length is admitted, every item
    below it is, and the runs cover every transform exactly once; the eight rows as one call find their waves"""
    out = run_check(tmp_path, "line_plan_check")
    m = re.fullmatch(r"line_plan_check: (\d+) cases, 0 failures\n", out)
    assert m, out[-2000:]
    assert int(m.group(1)) == 2048 * 2 * 9


def test_line_find_under_sanitizers(tmp_path):
    out = run_check(tmp_path, "line_find_check")
    m = re.fullmatch(r"line_find_check: (\d+) cases, 0 failures\n", out)
    assert m, out[-2000:]
    assert int(m.group(1)) >= 50


def test_simplest_ratio_against_brute_force_under_sanitizers(tmp_path):
    out = run_check(tmp_path, "ratio_check")
    m = re.fullmatch(r"ratio_check: (\d+) cases, 0 failures\n", out)
    assert m, out[-2000:]
    assert int(m.group(1)) >= 300 * 6
