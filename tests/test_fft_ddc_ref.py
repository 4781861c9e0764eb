"""The FftDdc's definition (tests/_fft_ddc_ref.py, csrc/hostlogic/fft_ddc_plan.hpp) against the Ddc's (tests/_ddc_ref.py), on
the CPU: with every image folded (R = D) the overlap-save form IS the Ddc's literal definition, to 1e-12 of the signal;
with R = 2 and R = 1 it stays inside the Cauchy-Schwarz bound on the bins the slice drops, computed from the response
tables; a float32 restatement in the definition's order stays inside the first-order device bound, so float32 arithmetic
can keep that bound; and the integer rotator phase equals its statement in fractions."""
import fractions

import numpy as np
import pytest

import _ddc_ref as dref
import _fft_ddc_ref as fref

N = fref.N
START = (1 << 40) + 3
# (D, V, K) of the issue, frequencies with a slice that wraps bin 0's far side (0.4999, -0.5)
EXACT_CASES = [(4, 64, 3), (16, 256, 2), (64, 1024, 2)]
FREQS = [0.4999, -0.5, 0.1234567]
# (D, V, R, K): the shapes of the device tests
DEVICE_CASES = [(4, 64, 2, 1), (16, 256, 2, 9), (64, 1024, 4, 3), (16, 1024, 16, 2), (32, 512, 1, 64)]


def stimulus(n, seed=5):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.25
    t = np.arange(n)
    return x + 0.7 * np.exp(2j * np.pi * 0.4999 * t) + 0.5 * np.exp(2j * np.pi * (-0.31) * t)


def taps_for(D, V):
    return dref.kaiser_taps64(D, min(12 * D, V + 1))


def device_freqs(K):
    """both sides of a 64-bin boundary, exactly on a bin, half-way between two bins, a slice across +-0.5, then a spread"""
    f = [63.4 / N, 64.3 / N, 200.0 / N, 300.5 / N, 0.4999, -0.5]
    rng = np.random.default_rng(11)
    return (f + list(rng.uniform(-0.5, 0.5, 64)))[:K] if K > 1 else [64.3 / N]


@pytest.mark.parametrize("D,V,K", EXACT_CASES)
def test_all_images_folded_is_the_ddc(D, V, K):
    hop = N - V
    x = stimulus(5 * hop + 77)
    h = taps_for(D, V)
    got = fref.fft_ddc64(x, h, D, FREQS[:K], V=V, R=D, start=START)
    want = dref.ddc64(x, h, D, FREQS[:K], start=START)
    assert got.shape == (K, fref.segments(x.size, D, V) * hop // D) and got.shape[1] > 0
    err = np.max(np.abs(got - want[:, :got.shape[1]]))
    print(f"D {D} V {V}: worst difference {err:.3e} of {np.max(np.abs(want)):.3f}")
    assert err <= 1e-12 * np.max(np.abs(want))


@pytest.mark.parametrize("R", [2, 1])
@pytest.mark.parametrize("D,V,K", EXACT_CASES)
def test_fewer_images_stay_inside_the_truncation_bound(D, V, K, R):
    hop = N - V
    x = stimulus(5 * hop + 77)
    h = taps_for(D, V)
    got = fref.fft_ddc64(x, h, D, FREQS[:K], V=V, R=R, start=START)
    want = dref.ddc64(x, h, D, FREQS[:K], start=START)[:, :got.shape[1]]
    bound = np.repeat(fref.truncation_bound(x, h, D, FREQS[:K], V, R), hop // D, axis=1)
    err = np.abs(got - want)
    print(f"D {D} V {V} R {R}: worst error / bound {np.max(err / bound):.3f}, worst error {np.max(err):.3e}")
    assert np.all(err <= bound + 1e-12 * np.max(np.abs(want)))


@pytest.mark.parametrize("D,V,R,K", DEVICE_CASES)
def test_float32_keeps_the_device_bound(D, V, R, K):
    hop = N - V
    x = stimulus(5 * hop + 77).astype(np.complex64)
    h = taps_for(D, V).astype(np.float32)
    f = device_freqs(K)
    got = fref.fft_ddc32(x, h, D, f, V, R, start=START)
    want = fref.fft_ddc64(x, h, D, f, V=V, R=R, start=START)
    bound = fref.device_bound(x, h, D, f, V, R)
    err = np.abs(got.astype(np.complex128) - want)
    print(f"D {D} V {V} R {R} K {K}: worst error / bound {np.max(err / bound):.3f}")
    assert got.shape == want.shape == bound.shape and got.shape[1] == 5 * hop // D
    assert np.all(err <= bound)


def test_rotator_phase_in_fractions():
    rng = np.random.default_rng(3)
    for f in FREQS + [64.5 / N, 0.0, 1.0 / 3.0] + list(rng.uniform(-0.5, 0.5, 50)):
        w = dref.frequency_word(f)
        c = fref.nearest_bin(w)
        assert c == int(fractions.Fraction(w * N, 1 << 32) + fractions.Fraction(1, 2)) % N  # floor of a non-negative value
        for i in [0, 1, START, (1 << 64) - 1] + [int(v) for v in rng.integers(0, 1 << 62, 5)]:
            for p in (0, 1, 16, 1024, 2047):
                turn = (fractions.Fraction(w * i, 1 << 32) - fractions.Fraction(c * p, N)) % 1
                assert fractions.Fraction(fref.phi(w, c, i, p), 1 << 32) == turn
