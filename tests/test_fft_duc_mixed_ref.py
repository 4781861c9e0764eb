"""The MixedFftDuc's definition (tests/_fft_duc_mixed_ref.py, csrc/hostlogic/fft_duc_mixed_plan.hpp) on the CPU: with every
image used (R_k = I_k) it is the sum of the Duc's literal definition (tests/_duc_ref.py) of each row alone, to 1e-12 of the
signal; with all I_k equal it is the FftDuc's definition (tests/_fft_duc_ref.py) to the last bit; with R = 2 and R = 1 it
stays inside the truncation bound; cut into calls of whole slots it is the definition of one call; and a float32
restatement in the definition's order stays inside the first-order device bound at every shape of the device tests."""
import functools

import numpy as np
import pytest

import _duc_ref as uref
import _fft_duc_mixed_ref as mref
import _fft_duc_ref as fref
import test_fft_duc_ref as uni

N = mref.N
START = uni.START
# (interpolations, V): mixed both ways round, and a pair of equal rows beside a faster one
EXACT_CASES = [((4, 16, 64), 1024), ((64, 8), 768), ((32, 32, 8), 512)]
CYCLE = (4, 8, 16, 32, 64)
# (interpolations, V, images): the shapes of the device tests.  The last has Bmax = 512, 64 rows and every group of four mixed
DEVICE_CASES = [((4, 16, 64, 8), 1024, (2, 2, 2, 2)), ((64, 4), 768, (4, 1)), ((32, 32, 8), 512, (32, 2, 8)),
                (tuple(CYCLE[k % 5] for k in range(64)), 768, (2,) * 64)]


def slots_for(Is, V):
    return 5 * ((N - V) // max(Is)) + 1


@functools.lru_cache(maxsize=None)
def rows_for(Is, V, slots=None):
    """section 27's stimulus, row k cut to its slots Imax / I_k items"""
    n = mref.items_for(Is, slots_for(Is, V) if slots is None else slots)
    v = uni.stimulus(len(Is), max(n))
    return [v[k, :n[k]] for k in range(len(Is))]


def taps_for(Is, V):
    return [uni.taps_for(I, V) for I in Is]


def freqs_for(K):
    return uni.FREQS[:K] if K <= 3 else uni.device_freqs(K)


def gains_for(K):
    return uni.GAINS[:K] if K <= 3 else uni.device_gains(K)


def duc_sum(rows, hs, Is, f, g, n):
    """sum_k Duc([f_k], I_k, taps = h_k, gains = [a_k])(v_k): the first n samples"""
    return sum(uref.duc64(rows[k][None, :], hs[k], Is[k], [f[k]], [g[k]], start=START)[:n] for k in range(len(Is)))


@pytest.mark.parametrize("Is,V", EXACT_CASES)
def test_all_images_is_the_sum_of_the_ducs(Is, V):
    rows, hs, f, g = rows_for(Is, V), taps_for(Is, V), freqs_for(len(Is)), gains_for(len(Is))
    got = mref.mixed_fft_duc64(rows, hs, Is, f, g, V=V, Rs=Is, start=START)
    want = duc_sum(rows, hs, Is, f, g, got.size)
    assert got.shape == want.shape == (5 * (N - V),)
    err = np.max(np.abs(got - want))
    print(f"I {Is} V {V}: worst difference {err:.3e} of {np.max(np.abs(want)):.3f}")
    assert err <= 1e-12 * np.max(np.abs(want))


@pytest.mark.parametrize("I,V,R,K", uni.DEVICE_CASES[:4])
def test_equal_interpolations_are_the_fft_duc_to_the_last_bit(I, V, R, K):
    v = uni.stimulus(K, 5 * ((N - V) // I) + 1)
    h, f, g = uni.taps_for(I, V), uni.device_freqs(K), uni.device_gains(K)
    got = mref.mixed_fft_duc64(list(v), [h] * K, [I] * K, f, g, V=V, Rs=R, start=START)
    want = fref.fft_duc64(v, h, I, f, g, V=V, R=R, start=START)
    assert got.shape == (5 * (N - V),) and np.array_equal(got, want)


@pytest.mark.parametrize("R", [2, 1])
@pytest.mark.parametrize("Is,V", EXACT_CASES)
def test_fewer_images_stay_inside_the_truncation_bound(Is, V, R):
    rows, hs, f, g = rows_for(Is, V), taps_for(Is, V), freqs_for(len(Is)), gains_for(len(Is))
    got = mref.mixed_fft_duc64(rows, hs, Is, f, g, V=V, Rs=R, start=START)
    want = duc_sum(rows, hs, Is, f, g, got.size)
    bound = np.repeat(mref.truncation_bound(rows, hs, Is, f, g, V, R), N - V)
    err = np.abs(got - want)
    print(f"I {Is} V {V} R {R}: worst error / bound {np.max(err / bound):.3f}, worst error {np.max(err):.3e}")
    assert got.shape == bound.shape == (5 * (N - V),)
    assert np.all(err <= bound)


@pytest.mark.parametrize("Is,V", EXACT_CASES)
def test_calls_of_any_whole_slots_are_one_call(Is, V):
    Imax = max(Is)
    hs_, Bs = (N - V) // Imax, N // Imax
    slots = slots_for(Is, V)
    assert 2 * hs_ + Bs + 1 < slots  # every cut below is a call of its own
    rows, hs, f, g = rows_for(Is, V), taps_for(Is, V), freqs_for(len(Is)), gains_for(len(Is))
    want = mref.mixed_fft_duc64(rows, hs, Is, f, g, V=V, Rs=2, start=START)
    ref = mref.MixedFftDuc64(hs, Is, f, g, V=V, Rs=2, start=START)
    got, at = [], 0
    for cut in (1, hs_ - 1, hs_, Bs + 1, slots):
        step = min(cut, slots - at)
        got.append(ref.process([v[at * Imax // I:(at + step) * Imax // I] for v, I in zip(rows, Is)]))
        at += step
        assert ref.pending == at % hs_
    assert got[0].size == 0 and got[1].size == (N - V)  # 1 slot: nothing; hop / Imax - 1 more: the first segment
    assert np.array_equal(np.concatenate(got), want)


@pytest.mark.parametrize("Is,V,Rs", DEVICE_CASES)
def test_float32_keeps_the_device_bound(Is, V, Rs):
    K = len(Is)
    rows = [r.astype(np.complex64) for r in rows_for(Is, V)]
    hs = [h.astype(np.float32) for h in taps_for(Is, V)]
    f, g = uni.device_freqs(K), uni.device_gains(K)
    got = mref.mixed_fft_duc32(rows, hs, Is, f, g, V, Rs, start=START)
    want = mref.mixed_fft_duc64(rows, hs, Is, f, g, V=V, Rs=Rs, start=START)
    bound = mref.device_bound(rows, hs, Is, f, g, V, Rs, start=START)
    err = np.abs(got.astype(np.complex128) - want)
    print(f"I {Is[:6]} V {V} R {Rs[:6]} K {K}: worst error / bound {np.max(err / bound):.3f}")
    assert got.shape == want.shape == bound.shape == (5 * (N - V),)
    assert np.all(err <= bound)
