"""The band designer behind gr4pm_band_filter_taps as a stand-alone program under UndefinedBehaviorSanitizer and
AddressSanitizer: tests/hostlogic/band_filter_design_check.cpp transforms the taps of csrc/hostlogic/band_filter_design.hpp
in double on 2^16 frequencies and holds |H(f) e^{2 pi j f c} - ideal(f)| to 2 n_bands 10^(-A / 20) at every frequency at least
half a transition width from every merged band edge, in both modes, for (L, A, bands) = (257, 60, one band), (1025, 60,
three bands, one across +-0.5), (1025, 40, one band of width 0.006 at 0) and (513, 80, two bands); the merging of
overlapping, touching and wrapping bands; stop + pass = delta to 1e-15; every refusal.  No GPU, no HIP, nothing loaded into
python."""
import re

from test_carrier_find_check import run_check


def test_band_filter_design_under_sanitizers(tmp_path):
    out = run_check(tmp_path, "band_filter_design_check")
    print(out)
    m = re.search(r"^band_filter_design_check: (\d+) cases, 0 failures\n\Z", out, re.M)
    assert m, out[-2000:]
    # four designs in two modes, the merging, the complements, the refusals
    assert int(m.group(1)) >= 8 + 9 + 9 + 19
    # every design reported its worst deviation (the program holds it to the rule, and to a tenth of a ripple from below:
    # a Kaiser design's ripple is of the order it was designed for, so the rule is not vacuous)
    assert len(re.findall(r"worst deviation ([0-9.]+) x", out)) == 8
