"""The MixedFftDdc's definition (tests/_fft_ddc_mixed_ref.py, csrc/hostlogic/fft_ddc_mixed_plan.hpp) on the CPU: with every
image folded (R_k = D_k) each row IS the Ddc's literal definition at its own D_k (tests/_ddc_ref.py), to 1e-12 of the
signal, although all channels share the segments anchored on Dmax; with all D_k equal it is the FftDdc's definition
(tests/_fft_ddc_ref.py); with R = 2 and R = 1 each row stays inside the Cauchy-Schwarz bound on the bins its slice drops;
and a float32 restatement in the definition's order stays inside the first-order device bound at the shapes of the device
tests, so float32 arithmetic can keep that bound.

Measured (n = 5 hop + 77, start 2^40 + 3): R_k = D_k at D = (4, 16, 64, 8), V = 1024: worst differences 9.0e-16, 5.6e-16,
1.8e-16, 3.0e-16 of signals 1.16, 0.87, 0.086, 0.29; equal decimations: no difference from fft_ddc64 at all; float32
over the device bound, worst per shape in DEVICE_CASES' order: 0.0026, 0.0119, 0.0051, 0.0106."""
import numpy as np
import pytest

import _ddc_ref as dref
import _fft_ddc_mixed_ref as mref
import _fft_ddc_ref as fref
import test_fft_ddc_ref as one

N = fref.N
START = one.START
FREQS = [0.4999, -0.5, 0.1234567, 0.12]
MIXED = ((4, 16, 64, 8), 1024)
FIVE = (4, 8, 16, 32, 64)
# (D_k, V, R_k): the shapes of the device tests
DEVICE_CASES = [((4, 16, 64, 8), 1024, (2, 2, 2, 2)), ((64, 4), 768, (4, 1)), ((32, 32, 8), 512, (32, 2, 8)),
                (tuple(FIVE[k % 5] for k in range(64)), 768, (2,) * 64)]
CASE_IDS = ["D4-16-64-8", "D64-4", "D32-32-8", "K64"]
stimulus = one.stimulus


def taps_for(Ds, V):
    """per channel the Kaiser design of 12 taps a phase, cut to what the overlap takes beside Dmax"""
    return [dref.kaiser_taps64(D, min(12 * D, V - (max(Ds) - D) + 1)) for D in Ds]


def freqs_for(K):
    return FREQS[:K] if K <= len(FREQS) else FREQS + one.device_freqs(K - len(FREQS))


def test_all_images_folded_is_the_ddc_of_every_channel():
    Ds, V = MIXED
    hop = N - V
    x = stimulus(5 * hop + 77)
    hs = taps_for(Ds, V)
    got = mref.mixed64(x, hs, Ds, FREQS, V=V, Rs=Ds, start=START)
    S = mref.segments(x.size, Ds, V)
    assert S == 5
    for k, D in enumerate(Ds):
        want = dref.ddc64(x, hs[k], D, [FREQS[k]], start=START)[0]
        assert got[k].shape == (S * hop // D,)
        err = np.max(np.abs(got[k] - want[:got[k].size]))
        print(f"D {D} V {V}: worst difference {err:.3e} of {np.max(np.abs(want)):.3f}")
        assert err <= 1e-12 * np.max(np.abs(want))


@pytest.mark.parametrize("D,V", [(4, 64), (16, 256), (64, 1024)])
def test_equal_decimations_are_the_fft_ddc(D, V):
    hop = N - V
    x = stimulus(5 * hop + 77)
    h = one.taps_for(D, V)
    for R in (D, 2):
        got = mref.mixed64(x, [h] * 4, [D] * 4, FREQS, V=V, Rs=R, start=START)
        want = fref.fft_ddc64(x, h, D, FREQS, V=V, R=R, start=START)
        assert mref.first_kept(D, D, V) == V // D and want.shape == (4, 5 * hop // D)
        err = np.max(np.abs(np.stack(got) - want))
        print(f"D {D} V {V} R {R}: worst difference {err:.3e}")
        assert err <= 1e-12 * np.max(np.abs(want))


@pytest.mark.parametrize("R", [2, 1])
def test_fewer_images_stay_inside_the_truncation_bound(R):
    Ds, V = MIXED
    hop = N - V
    x = stimulus(5 * hop + 77)
    hs = taps_for(Ds, V)
    got = mref.mixed64(x, hs, Ds, FREQS, V=V, Rs=R, start=START)
    bound = mref.truncation_bound(x, hs, Ds, FREQS, V, R)
    for k, D in enumerate(Ds):
        want = dref.ddc64(x, hs[k], D, [FREQS[k]], start=START)[0][:got[k].size]
        b = np.repeat(bound[k], hop // D)
        err = np.abs(got[k] - want)
        print(f"D {D} V {V} R {R}: worst error / bound {np.max(err / b):.3f}, worst error {np.max(err):.3e}")
        assert np.all(err <= b + 1e-12 * np.max(np.abs(want)))


@pytest.mark.parametrize("Ds,V,Rs", DEVICE_CASES, ids=CASE_IDS)
def test_float32_keeps_the_device_bound(Ds, V, Rs):
    hop = N - V
    x = stimulus(5 * hop + 77).astype(np.complex64)
    hs = [h.astype(np.float32) for h in taps_for(Ds, V)]
    f = freqs_for(len(Ds))
    got = mref.mixed32(x, hs, Ds, f, V, Rs, start=START)
    want = mref.mixed64(x, hs, Ds, f, V=V, Rs=Rs, start=START)
    bound = mref.device_bound(x, hs, Ds, f, V, Rs)
    worst = 0.0
    for k, D in enumerate(Ds):
        assert got[k].shape == want[k].shape == bound[k].shape == (5 * hop // D,)
        err = np.abs(got[k].astype(np.complex128) - want[k])
        worst = max(worst, float(np.max(err / bound[k])))
        assert np.all(err <= bound[k]), (k, D)
    print(f"D {Ds[:5]}{'...' if len(Ds) > 5 else ''} V {V}: worst error / bound {worst:.4f}")
