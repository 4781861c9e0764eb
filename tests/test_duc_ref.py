"""The Duc's float64 references (tests/_duc_ref.py) against each other, on the CPU: the definition (zero-stuff, filter,
mix, sum) and the rotated-taps form the kernel implements, also from start indices beyond 2^32; single samples with
Python integers; the scale of the GPU tests' bound; the host-only tap design; Duc -> Ddc in float64 returns a
band-limited row."""
import numpy as np
import pytest

import _ddc_ref as dref
import _duc_ref as uref

FREQS = [0.0, 0.5, -0.3137, 3.0 * 2.0 ** -32, 0.123456789, -0.05, 0.41, 1.0 / 3.0]
GAINS = [1.0, -0.5, 2.0, 0.75, 1.25, -1.0, 3.0, 0.125]


def rows(K, n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))


def taps(L, seed):
    return np.random.default_rng(seed).standard_normal(L)


@pytest.mark.parametrize("I,L,K", [(5, 60, 3), (3, 97, 2), (1, 1, 1), (64, 768, 8)])
@pytest.mark.parametrize("start", [0, (1 << 32) - 1000, (1 << 40) + 3])
def test_definition_equals_rotated_taps_form(I, L, K, start):
    P = -(-L // I)
    v = rows(K, 6 * P + 40, I + L)
    h = taps(L, K)
    for gains in (None, GAINS[:K]):
        a = uref.duc64(v, h, I, FREQS[:K], gains, start)
        b = uref.duc64_rotated(v, h, I, FREQS[:K], gains, start, frames_per_block=7)
        assert a.shape == b.shape == (v.shape[1] * I,)
        S = uref.window_scale(v, h, I, gains)
        assert np.all(np.abs(a - b) <= 1e-12 * S)
        assert np.max(np.abs(a)) > 0.1 * np.max(S)


@pytest.mark.parametrize("start", [0, (1 << 32) - 100, (1 << 40) + 3])
def test_direct_evaluation_with_python_integers(start):
    I, L, K = 5, 58, 3
    v = rows(K, 70, 7)   # 350 samples: crosses 2^32 at sample 100 for the second start
    h = taps(L, 8)
    samples = [0, 1, 4, 5, 6, 57, 58, 99, 100, 101, 230, 349]
    want = uref.duc64_direct(v, h, I, FREQS[2:2 + K], GAINS[:K], start, samples)
    S = uref.window_scale(v, h, I, GAINS[:K])[samples]
    for fn in (uref.duc64, uref.duc64_rotated):
        got = fn(v, h, I, FREQS[2:2 + K], GAINS[:K], start)[samples]
        assert np.all(np.abs(got - want) <= 1e-12 * S)
    if start:  # the start matters: from 0 the same rows give other values
        assert np.max(np.abs(uref.duc64(v, h, I, FREQS[2:2 + K], GAINS[:K], 0)[samples] - want)) > 1e-3 * np.max(S)


def test_window_scale():
    rng = np.random.default_rng(3)
    for I, L, K in [(5, 60, 2), (1, 1, 1), (3, 7, 2), (4, 2, 1), (16, 100, 3)]:
        n = 37
        v = rng.standard_normal((K, n)) * (rng.random((K, n)) < 0.2)
        h = rng.standard_normal(L)
        a = GAINS[:K]
        got = uref.window_scale(v, h, I, a)
        for j in range(n * I):
            m, r = divmod(j, I)
            ps = [p for p in range(-(-L // I)) if p * I + r < L]
            want = sum(abs(a[k]) * sum(abs(h[p * I + r]) for p in ps) *
                       max([abs(v[k, m - p]) for p in ps if m - p >= 0], default=0.0) for k in range(K))
            assert abs(got[j] - want) <= 1e-12 * max(want, 1e-300)


def test_tap_design():
    """gr4pm_duc_taps (host only): I times the stated Kaiser design, scaled in double and rounded to float32 once; the
    Ddc's floats where the scaling is exact; the refusals"""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    for I, P in [(1, 12), (3, 32), (4, 12), (5, 12), (1000, 2), (1, 1)]:
        h = pkg.duc_taps(I, P)
        assert h.dtype == np.float32 and h.size == I * P
        h64 = I * dref.kaiser_taps64(I, I * P)
        # one rounding to float32 of the double design (whose Bessel and sinc differ from numpy's in the last bits)
        assert np.all(np.abs(h - h64) <= dref.EPS32 * np.abs(h64) + 1e-12 * I)
        assert abs(float(np.sum(h.astype(np.float64))) - I) < 1e-6 * I
    for I, P in [(1, 12), (4, 12), (64, 12), (1024, 3)]:  # a power of two scales the Ddc's floats exactly
        assert np.array_equal(pkg.duc_taps(I, P).view(np.uint32), (pkg.ddc_taps(I, P) * np.float32(I)).view(np.uint32))
    d5 = pkg.ddc_taps(5, 12)
    assert np.any(pkg.duc_taps(5, 12) != d5 * np.float32(5))  # scaled in double, not after the rounding
    for bad in [(0, 12), (1025, 1), (5, 0), (1024, 9)]:
        with pytest.raises(pkg.Gr4pmError):
            pkg.duc_taps(*bad)
    with pytest.raises(pkg.Gr4pmError):
        pkg.duc_taps(5, 12, 0.75, 0.25)


@pytest.mark.parametrize("I,P,f", [(5, 12, 0.13), (4, 8, -0.37)])
def test_float64_loopback(I, P, f):
    """ddc64(duc64(v)) at one carrier, the same Kaiser design on both sides (DC gain I up, 1 down), returns a row that
    is band-limited to the design's passband (|f| <= 0.25 of the row's rate), delayed by the two filters' L - 1 wideband
    samples less the Ddc's D - 1, that is by P - 1 items.  The level: the design's ripple is delta = 10^(-A / 20) with
    the A of Kaiser's length rule that kaiser_taps64 uses; the passband passes both filters, (1 +- delta)^2, and every
    image or alias is attenuated twice, delta^2 each, so the RMS error is within 2 delta + O(delta^2) of the row's RMS:
    asserted at 3 delta."""
    L, n = I * P, 4096
    A = 2.285 * (2.0 * np.pi * 0.5 / I) * (L - 1) + 7.95
    delta = 10.0 ** (-A / 20.0)
    rng = np.random.default_rng(I)
    spec = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    spec[np.abs(np.fft.fftfreq(n)) > 0.25] = 0
    v = np.fft.ifft(spec)
    v /= np.sqrt(np.mean(np.abs(v) ** 2))
    h = dref.kaiser_taps64(I, L)
    start = (1 << 32) - 777
    y = dref.ddc64(uref.duc64(v, I * h, I, [f], None, start), h, I, [f], start)[0]
    lags = np.arange(0, 3 * P)
    mid = slice(4 * P, n - 4 * P)
    corr = [abs(np.vdot(v[mid], y[mid.start + lag:mid.stop + lag])) for lag in lags]
    lag = int(lags[int(np.argmax(corr))])
    assert lag == P - 1
    err = y[mid.start + lag:mid.stop + lag] - v[mid]
    rms = np.sqrt(np.mean(np.abs(err) ** 2))
    print(f"\n[duc loopback] I = {I}, P = {P}: A = {A:.1f} dB, delta = {delta:.3e}, rms error {rms:.3e} = {rms / delta:.3f} delta")
    assert rms <= 3.0 * delta
    assert rms > 1e-3 * delta  # the comparison is not vacuous: the ripple is there
