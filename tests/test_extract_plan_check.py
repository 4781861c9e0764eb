"""The host logic of Ddc.extract as a stand-alone program under UndefinedBehaviorSanitizer and AddressSanitizer:
tests/hostlogic/extract_plan_check.cpp sweeps csrc/hostlogic/extract_plan.hpp over D in {1, 2, 5, 16, 1000, 1024} x L in
{1, 60, 2000, 8192} with spans at frame 0, at the buffer's last frame, past its end and at 2^64 / D: every index the
kernel would stage lies in [0, 2^64), every in-buffer test is right, every refusal is the one the header states, and
burst_span() always covers [start_sample, end_sample).  No GPU, no HIP, nothing loaded into python.

Ddc.burst_spans() states burst_span() again in Python integers (ddc_burst_span): held here to the same covering property."""
import re

import numpy as np

import __graft_entry__ as ge
from test_carrier_find_check import run_check


def test_extract_plan_sweep_under_sanitizers(tmp_path):
    out = run_check(tmp_path, "extract_plan_check")
    m = re.fullmatch(r"extract_plan_check: (\d+) cases, 0 failures\n", out)
    assert m, out[-2000:]
    assert int(m.group(1)) >= 6 * 4 * 200 * 4


def test_ddc_burst_span_covers_the_burst():
    """every frame n whose samples [i - L + 1, i], i = start + n D + D - 1, touch [s, e) lies in the span, with the margin
    on either side where frame 0 does not stop it"""
    span = ge.load_package().ddc_burst_span
    rng = np.random.default_rng(7)
    for D in (1, 2, 5, 16, 1000, 1024):
        for L in (1, 60, 2000, 8192):
            for start in (0, 3, (1 << 40) + 3):
                for rep in range(40):
                    margin = 0 if rep % 4 == 0 else int(rng.integers(0, 1000))
                    s = int(rng.integers(0, start + 1)) if rep % 5 == 0 else start + int(rng.integers(0, 100000))
                    e = s + (0 if rep % 7 == 0 else 1 + int(rng.integers(0, 30000)))
                    first, n = span(s, e, D, L, start, margin)
                    if e <= s:
                        assert (first, n) == (0, 0)
                        continue
                    n_min = max(0, -(-(s - start - (D - 1)) // D))
                    n_max = (e - 1 - start - D + L) // D
                    if n_max < n_min:
                        continue
                    assert first <= max(0, n_min - margin) and first + n - 1 >= n_max + margin, (D, L, start, s, e, margin, first, n)
    assert span(10, 20, 5, 60, (1 << 64) - 3) == (0, 0)  # no frame of such a handle fits 64 bits
    first, n = span((1 << 64) - 4000, (1 << 64) - 1, 16, 60, 0, 10)
    assert (first + n) * 16 + 59 <= (1 << 64) - 2
