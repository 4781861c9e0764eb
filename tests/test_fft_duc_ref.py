"""The FftDuc's definition (tests/_fft_duc_ref.py, csrc/hostlogic/fft_duc_plan.hpp) against the Duc's (tests/_duc_ref.py), on
the CPU: with every image used (R = I) the overlap-save form IS the Duc's literal definition, to 1e-12 of the signal; with
R = 2 and R = 1 it stays inside the Cauchy-Schwarz bound on the bins the slices drop, computed from the response tables; a
float32 restatement in the definition's order stays inside the first-order device bound, so float32 arithmetic can keep
that bound; and the definition cut into calls is the definition of one call."""
import numpy as np
import pytest

import _ddc_ref as dref
import _duc_ref as uref
import _fft_duc_ref as fref

N = fref.N
START = (1 << 40) + 3
# (I, V) of the issue; frequencies with overlapping slices that wrap bin 0's far side (0.4999, -0.5)
EXACT_CASES = [(4, 64), (16, 256), (64, 1024)]
FREQS = [0.4999, -0.5, 0.1234567]
GAINS = [1.0, -0.6, 1.7]
# (I, V, R, K): the shapes of the device tests
DEVICE_CASES = [(4, 64, 2, 1), (16, 256, 2, 9), (64, 1024, 4, 3), (16, 1024, 16, 2), (32, 512, 1, 64)]


def items_for(I, V):
    return 5 * ((N - V) // I) + 3


def stimulus(K, n, seed=5):
    """[K, n]: noise plus two tones on every row, each row its own"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    v = (rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))) * 0.25
    for k in range(K):
        v[k] += 0.7 * np.exp(2j * np.pi * (0.11 + 0.013 * k) * t) + 0.5 * np.exp(2j * np.pi * (-0.31 + 0.007 * k) * t)
    return v


def taps_for(I, V):
    """the Duc's design (DC gain I) cut to what the overlap admits"""
    return I * dref.kaiser_taps64(I, min(12 * I, V + 1))


def device_freqs(K):
    """both sides of a 64-bin boundary, exactly on a bin, half-way between two bins, slices across +-0.5, then a spread"""
    f = [63.4 / N, 64.3 / N, 200.0 / N, 300.5 / N, 0.4999, -0.5]
    rng = np.random.default_rng(11)
    return (f + list(rng.uniform(-0.5, 0.5, 64)))[:K] if K > 1 else [64.3 / N]


def device_gains(K):
    return [(-1.0) ** k * (0.5 + 0.3 * (k % 5)) for k in range(K)]


@pytest.mark.parametrize("I,V", EXACT_CASES)
def test_all_images_is_the_duc(I, V):
    hop = N - V
    v = stimulus(3, items_for(I, V))
    h = taps_for(I, V)
    got = fref.fft_duc64(v, h, I, FREQS, GAINS, V=V, R=I, start=START)
    want = uref.duc64(v, h, I, FREQS, GAINS, start=START)[:got.size]
    assert got.shape == (5 * hop,)
    err = np.max(np.abs(got - want))
    print(f"I {I} V {V}: worst difference {err:.3e} of {np.max(np.abs(want)):.3f}")
    assert err <= 1e-12 * np.max(np.abs(want))


@pytest.mark.parametrize("R", [2, 1])
@pytest.mark.parametrize("I,V", EXACT_CASES)
def test_fewer_images_stay_inside_the_truncation_bound(I, V, R):
    hop = N - V
    v = stimulus(3, items_for(I, V))
    h = taps_for(I, V)
    got = fref.fft_duc64(v, h, I, FREQS, GAINS, V=V, R=R, start=START)
    want = uref.duc64(v, h, I, FREQS, GAINS, start=START)[:got.size]
    bound = np.repeat(fref.truncation_bound(v, h, I, FREQS, GAINS, V, R), hop)
    err = np.abs(got - want)
    print(f"I {I} V {V} R {R}: worst error / bound {np.max(err / bound):.3f}, worst error {np.max(err):.3e}")
    assert got.shape == bound.shape == (5 * hop,)
    assert np.all(err <= bound + 1e-12 * np.max(np.abs(want)))


@pytest.mark.parametrize("I,V,R,K", DEVICE_CASES)
def test_float32_keeps_the_device_bound(I, V, R, K):
    hop = N - V
    v = stimulus(K, items_for(I, V)).astype(np.complex64)
    h = taps_for(I, V).astype(np.float32)
    f, g = device_freqs(K), device_gains(K)
    got = fref.fft_duc32(v, h, I, f, g, V, R, start=START)
    want = fref.fft_duc64(v, h, I, f, g, V=V, R=R, start=START)
    bound = fref.device_bound(v, h, I, f, g, V, R, start=START)
    err = np.abs(got.astype(np.complex128) - want)
    print(f"I {I} V {V} R {R} K {K}: worst error / bound {np.max(err / bound):.3f}")
    assert got.shape == want.shape == bound.shape == (5 * hop,)
    assert np.all(err <= bound)


@pytest.mark.parametrize("I,V", EXACT_CASES)
def test_calls_of_any_length_are_one_call(I, V):
    hop_items, B = (N - V) // I, N // I
    n = items_for(I, V)
    v = stimulus(3, n)
    h = taps_for(I, V)
    want = fref.fft_duc64(v, h, I, FREQS, GAINS, V=V, R=2, start=START)
    ref = fref.FftDuc64(h, I, FREQS, GAINS, V=V, R=2, start=START)
    got, at = [], 0
    for cut in (1, hop_items - 1, hop_items, B + 1, n):
        step = min(cut, n - at)
        got.append(ref.process(v[:, at:at + step]))
        at += step
        assert ref.pending == at % hop_items
    assert got[0].size == 0 and got[1].size == (N - V)  # 1 item: nothing; hopI - 1 more: the first segment
    assert np.array_equal(np.concatenate(got), want)
