"""CPU-side checks of the Spectrogram block: the host-only burst finder (gr4pm_find_bursts) against the restatement
(tests/_spectrogram_ref.py), the restatement's own row and band arithmetic, and the row bound of tests/test_spectrogram.py
against a float32 numpy transform, so that the bound is one float32 arithmetic can keep.  No GPU."""
import numpy as np
import pytest

import _spectrogram_ref as gref
import _spectrum_ref as sref

N = gref.N


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    import os
    if not os.path.exists(os.path.join(ge.PKG_DIR, "libgr4pm_hip.so")):
        ge.build()
    return ge.load_package()


def series(T, runs, level=40.0, seed=3):
    """a noise floor around 1 with `runs` = [(first, length)] of rows at about `level`"""
    rng = np.random.default_rng(seed)
    p = 1.0 + 0.05 * rng.random(T)
    for a, n in runs:
        p[a:a + n] = level * (1.0 + 0.1 * rng.random(n))
    return p


def synthetic():
    """name -> (power, settings, the expected (first_row, n_rows) of every burst)"""
    c = {}
    c["all_inactive"] = (series(200, []), {}, [])
    c["flat"] = (np.full(50, 2.5), {}, [])
    c["one_run"] = (series(200, [(60, 9)]), {}, [(60, 9)])
    c["three_runs"] = (series(300, [(20, 5), (100, 17), (250, 3)]), {}, [(20, 5), (100, 17), (250, 3)])
    for gap, want in ((2, [(40, 12)]), (3, [(40, 5), (48, 5)])):  # a gap of exactly max_gap_rows merges, one more does not
        c[f"gap{gap}"] = (series(200, [(40, 5), (45 + gap, 5)]), dict(max_gap_rows=2), want)
    c["gap0_no_merge"] = (series(200, [(40, 5), (46, 5)]), dict(max_gap_rows=0), [(40, 5), (46, 5)])
    c["short_run"] = (series(200, [(30, 3), (90, 4)]), dict(min_rows=4), [(90, 4)])  # a run of min_rows - 1 is dropped
    c["bridged_counts"] = (series(200, [(30, 1), (32, 1)]), dict(min_rows=3, max_gap_rows=1), [(30, 3)])
    c["touches_row_0"] = (series(200, [(0, 6)]), {}, [(0, 6)])
    c["touches_last_row"] = (series(200, [(193, 7)]), {}, [(193, 7)])
    c["both_ends"] = (series(120, [(0, 4), (116, 4)]), {}, [(0, 4), (116, 4)])
    # more than half of the rows are active: the median is a burst row and finds nothing; an explicit floor finds the runs
    busy = series(100, [(5, 30), (50, 35)])
    c["busy_median"] = (busy, {}, [])
    c["explicit_floor"] = (busy, dict(floor=1.02), [(5, 30), (50, 35)])
    c["one_row_stream"] = (np.array([3.0]), dict(min_rows=1), [])
    return c


CASES = synthetic()


@pytest.mark.parametrize("name", sorted(CASES))
def test_find_bursts_against_restatement(pkg, name):
    p, kw, expected = CASES[name]
    want = gref.find_bursts(p, **kw)
    assert [(b["first_row"], b["n_rows"]) for b in want] == expected, want
    got = pkg.find_bursts(p, **kw)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for f in ("first_row", "n_rows", "peak_row"):
            assert int(g[f]) == w[f], (name, f)
        for f in ("power", "snr_db"):
            assert abs(float(g[f]) - w[f]) <= 1e-12 * abs(w[f]), (name, f, g[f], w[f])
        assert w["first_row"] <= w["peak_row"] < w["first_row"] + w["n_rows"]
    assert np.all(np.diff(got["first_row"].astype(np.int64)) > 0)


def test_burst_values():
    """the restatement against numbers worked out by hand: floor 1, rows 2 .. 4 and 6 at 11, 21, 21, 5"""
    p = np.array([1.0, 1.0, 11.0, 21.0, 21.0, 1.0, 5.0, 1.0, 1.0, 1.0, 1.0])
    (b,) = gref.find_bursts(p, threshold_db=3.0, max_gap_rows=1, min_rows=2)
    assert (b["first_row"], b["n_rows"], b["peak_row"]) == (2, 5, 3)  # the first row of the maximum; row 5 is bridged
    assert b["power"] == (10.0 + 20.0 + 20.0 + 0.0 + 4.0) / 5 and abs(b["snr_db"] - 10.0 * np.log10(21.0)) < 1e-12
    assert gref.spans([b], 3000, 4048, first_row=7) == [((7 + 2) * 3000, (7 + 2 + 4) * 3000 + 4048)]


def test_cap_smaller_than_count(pkg):
    import ctypes as C
    from gr4_packet_modem_amd import _abi
    p, kw, expected = CASES["three_runs"]
    every = pkg.find_bursts(p, **kw)
    assert len(every) == 3
    for cap in (0, 1, 2):
        got = pkg.find_bursts(p, cap=cap, **kw)
        assert len(got) == cap and np.array_equal(got, every[:cap])  # the earliest
        params = _abi.BurstParams(6.0, 0.0, 1, 2)
        out = np.zeros(max(cap, 1), dtype=_abi.BURST_DTYPE)
        count = C.c_size_t(99)
        assert pkg.lib().gr4pm_find_bursts(p.ctypes.data_as(C.c_void_p), p.size, C.byref(params),
                                           out.ctypes.data_as(C.c_void_p) if cap else None, cap, C.byref(count)) == 0
        assert count.value == 3  # the number found, even beyond cap


def test_find_bursts_refusals(pkg):
    import ctypes as C
    from gr4_packet_modem_amd import _abi
    p = np.ones(64)
    for bad in (0.0, -3.0, float("nan")):
        with pytest.raises(pkg.Gr4pmError):
            pkg.find_bursts(p, threshold_db=bad)
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(pkg.Gr4pmError):
            pkg.find_bursts(p, floor=bad)
    with pytest.raises(pkg.Gr4pmError):
        pkg.find_bursts(np.zeros(0))
    L, ptr = pkg.lib(), p.ctypes.data_as(C.c_void_p)
    params, out, count = _abi.BurstParams(6.0, 0.0, 1, 2), np.zeros(4, dtype=_abi.BURST_DTYPE), C.c_size_t(0)
    optr = out.ctypes.data_as(C.c_void_p)
    assert L.gr4pm_find_bursts(None, 64, C.byref(params), optr, 4, C.byref(count)) == -1  # GR4PM_ERR_INVALID
    assert L.gr4pm_find_bursts(ptr, 64, None, optr, 4, C.byref(count)) == -1
    assert L.gr4pm_find_bursts(ptr, 64, C.byref(params), optr, 4, None) == -1
    assert L.gr4pm_find_bursts(ptr, 64, C.byref(params), None, 4, C.byref(count)) == -1
    assert L.gr4pm_find_bursts(ptr, 0, C.byref(params), optr, 4, C.byref(count)) == -1


def test_rows_of_the_restatement():
    """row counts and the samples a row covers, from the definition"""
    for hop, R in ((2048, 1), (1000, 3), (1, 64), (512, 4)):
        for T in (0, 2047, 2048, 2048 + (R - 1) * hop - 1, 2048 + (R - 1) * hop, 2048 + (2 * R - 1) * hop):
            rows = gref.n_rows(T, hop, R)
            # rows fit, one more does not
            assert rows == 0 or (rows - 1) * R * hop + (R - 1) * hop + N <= T
            assert rows * R * hop + (R - 1) * hop + N > T
    x = gref.stimulus(40000)
    w = sref.hann()
    for det in gref.DETECTORS:
        r1, r3 = gref.rows(x, 1000, 1, det, w), gref.rows(x, 1000, 3, det, w)
        assert r1.shape == (38, N) and r3.shape == (12, N)
        want = r1[:36].reshape(12, 3, N)
        assert np.allclose(r3, want.mean(axis=1) if det == "mean" else want.max(axis=1), rtol=1e-13)
    assert np.array_equal(gref.rows(x, 1000, 1, "mean", w), gref.rows(x, 1000, 1, "max", w))  # R = 1: no detector


def test_band_power_of_the_restatement():
    r = np.arange(3 * N, dtype=np.float64).reshape(3, N)
    got = gref.band_power(r, [(100, 138), (2000, 138), (0, N), (77, 1)])
    assert got.shape == (4, 3)
    assert got[0, 1] == r[1, 100:238].sum() and got[1, 2] == r[2, 2000:].sum() + r[2, :90].sum()
    assert got[2, 0] == r[0].sum() and got[3, 1] == r[1, 77]


@pytest.mark.parametrize("kind", gref.KINDS)
@pytest.mark.parametrize("hop,n,R", gref.SHAPES)
def test_float32_fft_on_the_cpu_keeps_the_row_bound(hop, n, R, kind):
    """a float32 transform (numpy's, on complex64), the powers of a row summed (maximised) in float32 in segment order
    from the first power itself, one float32 product with fl32(inv): both detectors stay inside the bound that
    tests/test_spectrogram.py holds the kernel to, at every shape it uses"""
    x, w = gref.stimulus(n), gref.window_of(kind)
    T = gref.n_rows(n, hop, R)
    P = np.empty((T * R, N), dtype=np.float32)
    for s in range(T * R):
        X = np.fft.fft((w * x[s * hop: s * hop + N]).astype(np.complex64))
        assert X.dtype == np.complex64
        P[s] = X.real * X.real + X.imag * X.imag
    P = P.reshape(T, R, N)
    for det in gref.DETECTORS:
        inv = np.float32(1.0 / gref.normaliser(w, R, det))
        acc = P[:, 0].copy()
        for i in range(1, R):
            acc = acc + P[:, i] if det == "mean" else np.maximum(acc, P[:, i])
        got = acc * inv
        assert got.dtype == np.float32
        worst = gref.worst_over_bound(got, n, hop, R, det, kind)
        print(f"hop {hop} n {n} R {R} {kind} {det}: worst error / bound {worst:.3f}")
        assert worst <= 1.0
