"""The LineSpectrum block's definition without a GPU: the float64 restatement (tests/_line_spectrum_ref.py) keeps the
identities the definition rests on, a float32 restatement keeps the derived bound, and the host-only entry points
(gr4pm_find_line, gr4pm_simplest_ratio, resample_ratio, provisional_decimation) equal the restatement through the ABI."""
import functools

import numpy as np
import pytest

import _line_spectrum_ref as lref

N = lref.N


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    import os
    if not os.path.exists(os.path.join(ge.PKG_DIR, "libgr4pm_hip.so")):
        ge.build()
    return ge.load_package()


@functools.lru_cache(maxsize=None)
def stimulus(n, seed=7):
    """seeded Gaussian noise plus two tones, one of them off the bin grid"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    x = 0.5 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x += 0.8 * np.exp(2j * np.pi * 0.012345 * t) + 0.3 * np.exp(2j * np.pi * (-77.0 / 2048) * t)
    x = x.astype(np.complex64)
    x.setflags(write=False)
    return x


def test_segment_counts():
    for hop in (1, 256, 1000, 1024, 2048):
        assert lref.segments(0, hop) == 0
        for n in (1, 2047, 2048):
            assert lref.segments(n, hop) == 1
        assert lref.segments(2049, hop) == 2
        assert lref.segments(N + 3 * hop, hop) == 4
        assert lref.segments(N + 3 * hop + 1, hop) == 5


@pytest.mark.parametrize("hop", [2048, 1024, 1000, 256])
@pytest.mark.parametrize("n", [1, 2047, 2049, 5000, 9001])
def test_pairs_equal_the_direct_real_transforms(hop, n):
    """sum_p (|Z_p[k]|^2 + |Z_p[N - k]|^2) / 2 = sum_s |Y_s[k]|^2 for real y, odd segment counts included"""
    x, w = stimulus(9001), lref.hann()
    r = lref.row_spectrum(x, n, hop, w, "envelope", 0.75)
    direct = lref.envelope_direct(x, n, hop, w, 0.75)
    assert np.max(np.abs(r["acc"] - direct)) <= 1e-12 * np.max(direct)
    assert np.array_equal(r["out"], r["out"][(N - np.arange(N)) % N])


@pytest.mark.parametrize("k0", [0, 1, 63, 64, 511, 512])
def test_tones_peak_where_the_power_law_says(k0):
    x = np.exp(2j * np.pi * k0 * np.arange(3 * N) / N).astype(np.complex64)
    w = np.ones(N, dtype=np.float32)
    assert int(np.argmax(lref.row_spectrum(x, 3 * N, 2048, w, "fourth")["out"])) == (4 * k0) % N
    assert int(np.argmax(lref.row_spectrum(x, 3 * N, 2048, w, "square")["out"])) == (2 * k0) % N


def test_envelope_of_two_tones_peaks_at_their_difference():
    k1, k2 = 300, 177
    t = np.arange(3 * N)
    x = (np.exp(2j * np.pi * k1 * t / N) + 0.5 * np.exp(2j * np.pi * k2 * t / N)).astype(np.complex64)
    out = lref.row_spectrum(x, 3 * N, 2048, np.ones(N, dtype=np.float32), "envelope")["out"].copy()
    out[0] = 0.0  # the mean of |x|^2
    top = set(np.argsort(out)[-2:].tolist())
    assert top == {k1 - k2, N - (k1 - k2)}


@pytest.mark.parametrize("statistic", lref.STATISTICS)
@pytest.mark.parametrize("hop,n", [(2048, 40000), (1024, 40000), (1000, 5000), (256, 40000), (1024, 1), (1024, 2047)])
def test_float32_on_the_cpu_keeps_the_bound(statistic, hop, n):
    """the nonlinearity in float32, numpy's complex64 transform, the powers summed in float32 in runs of 64 transforms and
    then in float64: the derived bound is one that float32 arithmetic keeps"""
    x, w, g = stimulus(40000), lref.hann(), np.float32(0.8125)
    ref = lref.row_spectrum(x, n, hop, w, statistic, g)
    xs = x[:n]
    ux, uy = g * xs.real, g * xs.imag
    assert ux.dtype == np.float32
    if statistic == "envelope":
        y = (ux * ux + uy * uy).astype(np.complex64)
    else:
        re, im = ux * ux - uy * uy, np.float32(2.0) * ux * uy
        if statistic == "fourth":
            re, im = re * re - im * im, np.float32(2.0) * re * im
        y = (re + 1j * im).astype(np.complex64)
    S = ref["segments"]
    seg = np.zeros((S + 1, N), dtype=np.complex64)
    for s in range(S):
        part = y[s * hop: s * hop + N]
        seg[s, :part.size] = part
    if statistic == "envelope":
        ins = [(w * seg[2 * p].real + 1j * (w * seg[2 * p + 1].real)).astype(np.complex64) for p in range((S + 1) // 2)]
    else:
        ins = [(w * seg[s].real + 1j * (w * seg[s].imag)).astype(np.complex64) for s in range(S)]
    acc = np.zeros(N)
    for t0 in range(0, len(ins), lref.RUN):
        part = np.zeros(N, dtype=np.float32)
        for v in ins[t0:t0 + lref.RUN]:
            X = np.fft.fft(v)
            assert X.dtype == np.complex64
            part = part + (X.real * X.real + X.imag * X.imag)
        acc += part.astype(np.float64)
    if statistic == "envelope":
        acc = lref.fold(acc)
    err = np.abs(acc - ref["acc"])
    print(f"{statistic} hop {hop} n {n}: worst error / bound {lref.worst_ratio(err, ref['bound']):.3f}")
    assert np.all(err <= ref["bound"])


def same_line(got, want):
    for f in ("bin", "found"):
        assert int(got[f]) == want[f], f
    for f in ("frequency", "snr_db", "margin_db", "peak", "floor"):
        g, w = float(got[f]), want[f]
        assert g == w or abs(g - w) <= 1e-12 * max(1.0, abs(w)), (f, g, w)


@pytest.mark.parametrize("seed", range(6))
def test_find_line_equals_the_restatement(pkg, seed):
    rng = np.random.default_rng(seed)
    n = (2048, 2048, 64, 100, 7, 2048)[seed]
    sp = rng.exponential(size=n)
    if seed % 2:
        sp[rng.integers(n)] = 40.0
    windows = [(0, n), (n - 3, min(n, 9)), (n // 2, 7), (1, n - 1)]
    for first, bins in windows:
        if bins < 7:
            continue
        same_line(pkg.find_line(sp, first, bins), lref.find_line(sp, first, bins))
    same_line(pkg.find_line(sp), lref.find_line(sp))
    same_line(pkg.find_line(sp, 2, 3, guard_bins=0), lref.find_line(sp, 2, 3, 0))


def test_find_line_special_spectra(pkg):
    flat = np.ones(64)
    r = pkg.find_line(flat, 60, 10)
    assert int(r["bin"]) == 60 and float(r["margin_db"]) == 0.0 and float(r["frequency"]) == 60 / 64 - 1
    same_line(r, lref.find_line(flat, 60, 10))
    zeros = np.zeros(64)
    r = pkg.find_line(zeros)
    assert int(r["found"]) == 0 and float(r["snr_db"]) == 0.0 and float(r["margin_db"]) == 0.0
    one = np.zeros(64)
    one[5] = 2.0  # neighbours are 0: no interpolation; floor and other are 0: infinite ratios
    r = pkg.find_line(one)
    assert int(r["found"]) == 1 and float(r["frequency"]) == 5 / 64 and np.isinf(float(r["margin_db"]))
    same_line(r, lref.find_line(one))
    # an exact parabola in the logarithm: a Gaussian line at 20.3
    k = np.arange(64, dtype=np.float64)
    g = np.exp(-0.5 * (k - 20.3) ** 2)
    assert abs(float(pkg.find_line(g)["frequency"]) - 20.3 / 64) < 1e-12
    for bad in [dict(first_bin=64), dict(n_bins=65), dict(n_bins=6), dict(n_bins=4, guard_bins=1)]:
        with pytest.raises(pkg.Gr4pmError):
            pkg.find_line(flat, **bad)


def test_simplest_ratio_equals_the_restatement_on_a_grid(pkg):
    rng = np.random.default_rng(3)
    values = list(np.exp(rng.uniform(np.log(1e-3), np.log(50.0), size=200))) + [0.16, 1 / 3, 4 / 25, 0.5, 1.0, 2.5, 63.9, 1e-3]
    for v in values:
        for tol in (2e-3, 1e-4, 0.05):
            want = lref.simplest_ratio(v, tol, 64, 1024)
            if want is None:
                with pytest.raises(pkg.Gr4pmError):
                    pkg.simplest_ratio(v, tol, 64, 1024)
            else:
                got = pkg.simplest_ratio(v, tol, 64, 1024)
                assert got == want, (v, tol)
                assert np.gcd(*got) == 1
    for bad in [(0.0, 1e-3), (-1.0, 1e-3), (np.nan, 1e-3), (np.inf, 1e-3), (0.5, -1e-3), (0.5, np.nan), (0.5, 1.0)]:
        with pytest.raises(pkg.Gr4pmError):
            pkg.simplest_ratio(bad[0], bad[1], 64, 1024)
    with pytest.raises(pkg.Gr4pmError):
        pkg.simplest_ratio(0.5, 1e-3, 0, 10)


def test_resample_ratio_and_provisional_decimation(pkg):
    assert pkg.resample_ratio(0.04) == (4, 25)
    assert pkg.resample_ratio(1 / 12) == (1, 3)
    assert pkg.resample_ratio(0.04 * (1 + 1.5e-3)) == (4, 25)
    with pytest.raises(pkg.Gr4pmError):
        pkg.resample_ratio(0.0401234, rel_tol=1e-6)  # no fraction with I <= 64 and D <= 1024 is that close
    assert pkg.provisional_decimation(0.054) == 7
    assert pkg.provisional_decimation(0.9) == 1
    with pytest.raises(pkg.Gr4pmError):
        pkg.provisional_decimation(0.0)


def test_the_library_exports_the_new_entry_points(pkg):
    for name in ("gr4pm_line_spectrum_float_run", "gr4pm_line_spectrum_create", "gr4pm_line_spectrum_destroy",
                 "gr4pm_line_spectrum_process", "gr4pm_find_line", "gr4pm_simplest_ratio"):
        assert hasattr(pkg.lib(), name)
    assert pkg.lib().gr4pm_line_spectrum_float_run() == lref.RUN
