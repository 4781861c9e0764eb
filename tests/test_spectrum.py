"""The Spectrum block on the GPU against the float64 restatement of its definition (tests/_spectrum_ref.py) within a
derived bound, and its exact properties: the lane / register to bin layout, power-of-two scaling, call cuts, short
streams, integer ingest, refusals.

The bound.  With X64_s the float64 transform of segment s and delta_s = 8 * 2^-24 * ||X64_s||_2 (C = 8 is what
tests/test_syncword_float64.py holds every GPU form of this transform to), per bin
    |acc32[k] - acc64[k]| <= sum_s (2 |X64_s[k]| delta_s + delta_s^2) + R * 2^-24 * acc64[k]
    |max32[k] - max64[k]| <= max_s (2 |X64_s[k]| delta_s + delta_s^2)
|X32|^2 - |X64|^2 = 2 Re(conj(X64) e) + |e|^2 with |e| <= delta_s; R = 64 = gr4pm_spectrum_float_run() is the number of
powers a wave adds in float32 before the sum goes on in float64.  First order, worst case: not a fit."""
import ctypes as C
import functools

import numpy as np
import pytest

import _spectrum_ref as sref
from _frontend import dev, exact_iq_forms, load_package

pytestmark = pytest.mark.gpu

N = 2048
RUN = 64
CUTS = (1, 63, 2048, 4097)


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@functools.lru_cache(maxsize=None)
def stimulus(n, seed=5):
    """seeded Gaussian noise plus two tones, one of them off the bin grid"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    x = 0.5 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x += 0.8 * np.exp(2j * np.pi * 0.12345 * t) + 0.3 * np.exp(2j * np.pi * (-777.0 / 2048) * t)
    x = x.astype(np.complex64)
    x.setflags(write=False)
    return x


def window_of(kind):
    return None if kind == "hann" else np.ones(N, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def reference(n, hop, kind):
    """the float64 result and the two bounds, computed once per (stream, hop, window)"""
    w = sref.hann() if kind == "hann" else np.ones(N, dtype=np.float32)
    r = sref.welch(stimulus(n), hop, w)
    r["acc_bound"], r["max_bound"] = sref.bounds(r["X"], RUN)
    return r


def run(pkg, x, hop, kind="hann", cuts=(), scale=None, sp=None):
    """x (numpy complex64, or integer IQ [n, 2]) through a Spectrum in calls of the lengths `cuts`, then the rest"""
    sp = sp or pkg.Spectrum(hop=hop, window=window_of(kind))
    d, lo = dev(x), 0
    for c in cuts:
        sp.process_bulk(d[lo:lo + c], scale=scale) if scale is not None else sp.process_bulk(d[lo:lo + c])
        lo = min(lo + c, len(x))
    if lo < len(x) or not cuts:
        sp.process_bulk(d[lo:], scale=scale) if scale is not None else sp.process_bulk(d[lo:])
    return sp.read()


def assert_within_bound(got, ref):
    S, wp = ref["segments"], ref["window_power"]
    assert got["segments"] == S
    if S == 0:
        assert not got["mean"].any() and not got["max_hold"].any()
        return
    acc_err = np.abs(got["mean"] - ref["mean"]) * (S * wp)
    max_err = np.abs(got["max_hold"].astype(np.float64) * wp - ref["max"])
    print(f"acc: worst error / bound {np.max(acc_err / ref['acc_bound']):.3f}   "
          f"max: worst error / bound {np.max(max_err / ref['max_bound']):.3f}   segments {S}")
    assert np.all(acc_err <= ref["acc_bound"])
    assert np.all(max_err <= ref["max_bound"])


# (hop, samples): at hop 1 the stream the specification names, and one whose 8192 segments make runs of four per wave
SHAPES = [(2048, 40000), (1024, 40000), (1000, 40000), (1, 2048 + 300), (1, 2048 + 8191)]


def test_float_run_is_the_bound_s(pkg):
    assert pkg.lib().gr4pm_spectrum_float_run() == RUN


@pytest.mark.parametrize("kind", ["hann", "rect"])
@pytest.mark.parametrize("hop,n", SHAPES)
def test_float32_fft_on_the_cpu_reaches_the_bound(hop, n, kind):
    """a float32 transform (numpy's, on complex64) with the powers summed in float32 in runs of 64, then in float64:
    the bound is one that float32 arithmetic can keep"""
    ref = reference(n, hop, kind)
    w = sref.hann() if kind == "hann" else np.ones(N, dtype=np.float32)
    x, S = stimulus(n), ref["segments"]
    acc, mx = np.zeros(N), np.zeros(N, dtype=np.float32)
    for s0 in range(0, S, RUN):
        part = np.zeros(N, dtype=np.float32)
        for s in range(s0, min(s0 + RUN, S)):
            X = np.fft.fft((w * x[s * hop: s * hop + N]).astype(np.complex64))
            assert X.dtype == np.complex64
            p = X.real * X.real + X.imag * X.imag
            part = part + p
            mx = np.maximum(mx, p)
        acc += part.astype(np.float64)
    assert np.all(np.abs(acc - ref["acc"]) <= ref["acc_bound"])
    assert np.all(np.abs(mx.astype(np.float64) - ref["max"]) <= ref["max_bound"])


@pytest.mark.parametrize("kind", ["hann", "rect"])
@pytest.mark.parametrize("hop,n", SHAPES)
def test_within_the_float64_bound(pkg, hop, n, kind):
    assert_within_bound(run(pkg, stimulus(n), hop, kind), reference(n, hop, kind))


def test_white_noise_reads_its_power(pkg):
    """sigma^2 = 0.5 in every bin of mean, within the spread of an average of 38 segments (loosely: a gross scaling
    error is a factor of 2048 or 768)"""
    rng = np.random.default_rng(1)
    x = (0.5 * (rng.standard_normal(40000) + 1j * rng.standard_normal(40000))).astype(np.complex64)
    m = run(pkg, x, 1024)["mean"]
    assert abs(np.mean(m) - 0.5) < 0.02


@pytest.mark.parametrize("k0", [0, 1, 63, 64, 1023, 1024, 2047])
def test_layout_one_tone_at_a_bin_centre(pkg, k0):
    x = np.exp(2j * np.pi * k0 * np.arange(3 * N) / N).astype(np.complex64)
    r = run(pkg, x, 2048, "rect")
    assert r["segments"] == 3
    assert int(np.argmax(r["mean"])) == k0 and int(np.argmax(r["max_hold"])) == k0
    assert abs(r["mean"][k0] - N) < 1e-3 * N  # |X[k0]|^2 / sum w^2 = N^2 / N
    assert np.sum(r["mean"]) - r["mean"][k0] < 1e-6 * N


def test_power_of_two_scaling_is_exact(pkg):
    x = stimulus(40000)
    base = run(pkg, x, 1000)
    for e in (10, -10):
        r = run(pkg, (x * np.float32(2.0 ** e)).astype(np.complex64), 1000)
        assert np.array_equal(r["mean"], base["mean"] * 4.0 ** e)
        assert np.array_equal(r["max_hold"], base["max_hold"] * np.float32(4.0 ** e))


@pytest.mark.parametrize("hop", [2048, 1024, 1000, 1])
def test_call_cuts(pkg, hop):
    n = 2048 + 8191 if hop == 1 else 40000
    x, ref = stimulus(n), reference(n, hop, "hann")
    whole = run(pkg, x, hop)
    sp = pkg.Spectrum(hop=hop)
    cut = run(pkg, x, hop, cuts=CUTS, sp=sp)
    assert cut["segments"] == whole["segments"] == ref["segments"]
    # max is associative, and a segment's powers do not depend on where a call ended
    assert np.array_equal(cut["max_hold"].view(np.uint32), whole["max_hold"].view(np.uint32))
    assert_within_bound(cut, ref)
    # the same calls again give the same bits
    sp.reset()
    again = run(pkg, x, hop, cuts=CUTS, sp=sp)
    assert again["segments"] == cut["segments"]
    assert np.array_equal(again["mean"].view(np.uint64), cut["mean"].view(np.uint64))
    assert np.array_equal(again["max_hold"].view(np.uint32), cut["max_hold"].view(np.uint32))


def test_more_segments_than_one_launch_holds(pkg):
    """2048 waves of 64 segments are one launch: 135 000 segments in one call take two, in calls of 60 000 samples one
    each.  No reference at this size: the maxima must agree bit for bit, the means to the float32 sums' rounding."""
    rng = np.random.default_rng(9)
    n = N + 135000
    x = (0.5 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    whole = run(pkg, x, 1)
    cut = run(pkg, x, 1, cuts=(60000, 60000))
    assert whole["segments"] == cut["segments"] == 135001
    assert np.array_equal(cut["max_hold"].view(np.uint32), whole["max_hold"].view(np.uint32))
    assert np.all(np.abs(cut["mean"] - whole["mean"]) <= 2 * RUN * 2.0 ** -24 * whole["mean"])


def test_short_streams(pkg):
    x = stimulus(40000)[:N]
    sp = pkg.Spectrum(hop=1000)
    d = dev(x)
    r = sp.process_bulk(d[:0]).process_bulk(d[:N - 1]).read()
    assert r["segments"] == 0 and not r["mean"].any() and not r["max_hold"].any()
    assert r["mean"].dtype == np.float64 and r["max_hold"].dtype == np.float32 and r["mean"].shape == r["max_hold"].shape == (N,)
    r = sp.process_bulk(d[N - 1:]).read()  # the 2048th sample, in a call of its own
    assert r["segments"] == 1
    ref = sref.welch(x, 1000, sref.hann())
    ref["acc_bound"], ref["max_bound"] = sref.bounds(ref["X"], RUN)
    assert_within_bound(r, ref)
    assert np.array_equal(sp.frequencies, np.where(np.arange(N) < N // 2, np.arange(N), np.arange(N) - N) / N)


@pytest.mark.parametrize("form", [1, 2, 3], ids=["sc16", "sc8", "cu8"])
def test_integer_iq_equals_unpacked(pkg, form):
    _, forms = exact_iq_forms(20000, seed=3)
    v, scale = forms[form]
    got = run(pkg, v, 1000, cuts=CUTS, scale=scale)
    unpacked = pkg.iq_unpack(dev(v), scale=scale).cpu().numpy()
    want = run(pkg, unpacked, 1000, cuts=CUTS)
    assert got["segments"] == want["segments"] == sref.segments(20000, 1000)
    assert np.array_equal(got["mean"].view(np.uint64), want["mean"].view(np.uint64))
    assert np.array_equal(got["max_hold"].view(np.uint32), want["max_hold"].view(np.uint32))
    # a scale that is no power of two: the unpack rounds, the same way in both
    got = run(pkg, v, 1000, cuts=CUTS, scale=0.0123)
    want = run(pkg, pkg.iq_unpack(dev(v), scale=0.0123).cpu().numpy(), 1000, cuts=CUTS)
    assert np.array_equal(got["mean"].view(np.uint64), want["mean"].view(np.uint64))
    assert np.array_equal(got["max_hold"].view(np.uint32), want["max_hold"].view(np.uint32))


def test_formats_mix_on_one_handle(pkg):
    x, forms = exact_iq_forms(20000, seed=4)
    want = run(pkg, x, 1000, cuts=CUTS)
    sp = pkg.Spectrum(hop=1000)
    devs = [(dev(v), s) for v, s in forms]
    lo = 0
    for i, c in enumerate(CUTS + (3000, 500, 20000)):
        v, s = devs[i % 4]
        sp.process_bulk(v[lo:lo + c], scale=s) if s is not None else sp.process_bulk(v[lo:lo + c])
        lo = min(lo + c, 20000)
    got = sp.read()
    assert got["segments"] == want["segments"]
    assert np.array_equal(got["max_hold"].view(np.uint32), want["max_hold"].view(np.uint32))
    ref = sref.welch(x, 1000, sref.hann())
    ref["acc_bound"], ref["max_bound"] = sref.bounds(ref["X"], RUN)
    assert_within_bound(got, ref)


def test_refusals(pkg):
    from gr4_packet_modem_amd import _abi
    L = pkg.lib()
    nan_window = np.ones(N, dtype=np.float32)
    nan_window[1500] = np.nan
    inf_window = np.ones(N, dtype=np.float32)
    inf_window[0] = np.inf
    for fft_size, hop, window in ((2048, 0, None), (2048, 2049, None), (1024, 512, None), (4096, 1024, None),
                                  (2048, 1024, nan_window), (2048, 1024, inf_window)):
        h = C.c_void_p(0x1234)
        p = _abi.SpectrumParams(fft_size, hop, None if window is None else window.ctypes.data_as(C.c_void_p), None)
        assert L.gr4pm_spectrum_create(C.byref(p), C.byref(h)) == -1, (fft_size, hop)  # GR4PM_ERR_INVALID
        assert h.value is None
    for kw in (dict(hop=0), dict(hop=2049), dict(fft_size=1024), dict(window=nan_window)):
        with pytest.raises(pkg.Gr4pmError):
            pkg.Spectrum(**kw)
    sp = pkg.Spectrum(hop=2048)  # the largest hop is fine
    assert sp.read()["segments"] == 0
