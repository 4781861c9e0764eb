"""CPU-side checks of the Spectrum block: the restatement's segment counts (tests/_spectrum_ref.py), the window design
bit for bit, and the host-only carrier finder (gr4pm_find_carriers) against the restatement.  No GPU."""
import numpy as np
import pytest

import _spectrum_ref as sref


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    import os
    if not os.path.exists(os.path.join(ge.PKG_DIR, "libgr4pm_hip.so")):
        ge.build()
    return ge.load_package()


@pytest.mark.parametrize("hop", [1, 512, 1000, 1024, 2047, 2048])
def test_segment_counts(hop):
    N = sref.N
    for T in (0, 1, 2047, 2048, 2048 + hop - 1, 2048 + hop):
        S = sref.segments(T, hop)
        # S segments fit, one more does not
        assert S == 0 or (S - 1) * hop + N <= T
        assert S * hop + N > T
        assert S == sum(1 for s in range(T) if s * hop + N <= T)
    assert sref.segments(2047, hop) == 0 and sref.segments(2048, hop) == 1
    assert sref.segments(2048 + hop - 1, hop) == 1 and sref.segments(2048 + hop, hop) == 2


def test_window_bit_for_bit(pkg):
    n = np.arange(2048, dtype=np.float64)
    want = (0.5 - 0.5 * np.cos(2.0 * np.pi * n / 2048)).astype(np.float32)
    got = pkg.spectrum_window(2048)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(sref.hann().view(np.uint32), want.view(np.uint32))


def bump(psd, centre, width, height):
    """a raised-cosine carrier of `width` bins around bin `centre` on the circle"""
    n = psd.size
    for i in range(width):
        psd[(centre - width // 2 + i) % n] += height * (0.6 + 0.4 * np.sin(np.pi * (i + 0.5) / width))


def synthetic():
    """name -> (psd, settings, expected count)"""
    rng = np.random.default_rng(11)
    n = 2048
    base = lambda: 1.0 + 0.05 * rng.random(n)
    cases = {}
    p = base(); bump(p, 300, 41, 30.0)
    cases["one"] = (p, {}, 1)
    p = base(); bump(p, 1400, 60, 12.0); bump(p, 260, 31, 100.0); bump(p, 900, 45, 40.0)
    cases["three"] = (p, {}, 3)
    p = base(); bump(p, 1024, 50, 25.0)  # across +-0.5: bins 999 .. 1048
    cases["nyquist"] = (p, {}, 1)
    p = base(); bump(p, 3, 40, 25.0)     # across bin 0: bins 2031 .. 22
    cases["wrap_zero"] = (p, {}, 1)
    for gap, want in ((2, 1), (3, 2)):
        p = np.ones(n); p[100:110] = 50.0; p[110 + gap:120 + gap] = 60.0
        cases[f"gap{gap}"] = (p, dict(max_gap_bins=2), want)
    p = np.ones(n); p[500:503] = 40.0; p[700:704] = 40.0
    cases["narrow"] = (p, dict(min_width_bins=4), 1)
    cases["flat"] = (np.full(n, 3.25), {}, 0)
    cases["flat_noise"] = (1.0 + 0.05 * rng.random(n), {}, 0)
    p = base(); bump(p, 2040, 30, 25.0); bump(p, 600, 30, 25.0)  # one run wraps bin 0, another stands alone
    cases["wrap_and_one"] = (p, {}, 2)
    p = np.ones(257); p[250:257] = 9.0; p[0:3] = 9.0; p[120:131] = 20.0  # an odd n
    cases["odd_n"] = (p, {}, 2)
    return cases


CASES = synthetic()


@pytest.mark.parametrize("name", sorted(CASES))
def test_find_carriers_against_restatement(pkg, name):
    psd, kw, count = CASES[name]
    want = sref.find_carriers(psd, **kw)
    assert len(want) == count, want
    got = pkg.find_carriers(psd, **kw)
    assert len(got) == count and pkg.count_carriers(psd, **kw) == count
    for g, w in zip(got, want):
        assert int(g["first_bin"]) == w["first_bin"] and int(g["n_bins"]) == w["n_bins"]
        for f in ("frequency", "bandwidth", "power", "snr_db"):
            assert abs(float(g[f]) - w[f]) <= 1e-12 * abs(w[f]), (name, f, g[f], w[f])
        assert -0.5 <= g["frequency"] < 0.5
    assert np.all(np.diff(got["frequency"]) > 0)


def test_wrap_is_one_run(pkg):
    psd, kw, _ = CASES["nyquist"]
    (c,) = pkg.find_carriers(psd, **kw)
    assert int(c["first_bin"]) == 999 and int(c["n_bins"]) == 50
    assert abs(abs(c["frequency"]) - 0.5) < 2.0 / 2048
    psd, kw, _ = CASES["wrap_zero"]
    (c,) = pkg.find_carriers(psd, **kw)
    assert int(c["first_bin"]) == 2031 and int(c["n_bins"]) == 40 and abs(c["frequency"] - 3.0 / 2048) < 1.0 / 2048


def test_cap_smaller_than_count(pkg):
    psd, kw, count = CASES["three"]
    every = pkg.find_carriers(psd, **kw)
    for cap in (0, 1, 2):
        got = pkg.find_carriers(psd, cap=cap, **kw)
        assert len(got) == cap and pkg.count_carriers(psd, **kw) == count
        assert np.array_equal(got, every[:cap])  # the lowest frequencies


def test_refusals(pkg):
    psd = np.ones(64)
    for bad in (0.0, -3.0, float("nan")):
        with pytest.raises(pkg.Gr4pmError):
            pkg.find_carriers(psd, threshold_db=bad)
    with pytest.raises(pkg.Gr4pmError):
        pkg.find_carriers(np.zeros(0))
