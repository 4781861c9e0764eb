"""The RowResampler's definition on the CPU (no GPU): tests/_row_resampler_ref.py's float64 restatement against the
literal definition in fractions.Fraction and against the rational Ddc's definition, the output length against brute force,
the float32 restatement against section 24's error bound, theta against Python integers, and the host-only entry points
(the taps helper, output_lengths, tile_items)."""
from fractions import Fraction

import numpy as np
import pytest

import __graft_entry__ as ge
import _ddc_rational_ref as rref
import _row_resampler_ref as ref

TWO32 = 1 << 32


def _row(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def _taps(Q, P, seed=None):
    if seed is None:
        return ref.kaiser_taps64(Q, P).astype(np.float32)
    return np.random.default_rng(seed).standard_normal(Q * P).astype(np.float32)


@pytest.mark.parametrize("Q,P,step,phase0", [(32, 12, round(0.8929 * TWO32), 0), (4, 3, round(2.2727 * TWO32), TWO32 // 2),
                                             (256, 2, TWO32 + 1, 3 * TWO32 + TWO32 // 4), (2, 1, TWO32 // 64, 0)])
def test_restatement_against_the_literal_definition(Q, P, step, phase0):
    n = 40
    x, h = _row(n, 1), _taps(Q, P, seed=2)
    y = ref.resample64(x, n, h, Q, step, phase0)
    M = ref.output_items(n, P, step, phase0)
    assert y.size == M and M > 0
    scale = np.sum(np.abs(h)) / Q * np.max(np.abs(x))
    for m in sorted(set(np.linspace(0, M - 1, 25).astype(int).tolist())):
        lit = ref.literal(x, n, h, Q, Fraction(phase0 + m * step, TWO32))
        # Dh is rounded to float32 once, the literal difference is exact: 2^-24 of a tap's size per term
        assert abs(y[m] - lit) <= 4 * ref.EPS32 * scale * P + 1e-13 * scale, (m, y[m], lit)


def test_equals_the_rational_ddc_at_4_over_25():
    """Q = I = 4, step = 25 / 4, phase0 = 24 / 4, freq = 0: item n is the rational Ddc's item n (section 18)"""
    I, D, P, n = 4, 25, 9, 700
    x, h = _row(n, 3), _taps(I, P, seed=4)
    y = ref.resample64(x, n, h, I, D * TWO32 // I, (D - 1) * TWO32 // I)
    want = rref.rddc64(x, h.astype(np.float64), I, D, [0.0])[0]
    assert want.size == n * I // D and y.size >= want.size
    assert np.max(np.abs(y[:want.size] - want)) <= 1e-12 * np.sum(np.abs(h)) * np.max(np.abs(x))


def test_output_items_against_brute_force():
    pkg = ge.load_package()
    for P in (1, 12, 128):
        rs = pkg.RowResampler(phases=2, taps=np.ones(2 * P, np.float32))
        for step in (1 << 26, TWO32 - 1, TWO32, TWO32 + 1, round(0.893 * TWO32), 1 << 38):
            for n in (0, 1, max(P - 1, 0), P, 255):
                for phase0 in (0, 1 << 31, 3 * TWO32 + TWO32 // 4, (n + P + 5) << 32):
                    M = ref.output_items(n, P, step, phase0)
                    if n:
                        brute = 0
                        while ((phase0 + brute * step) >> 32) <= n + P - 2:
                            brute += 1
                        assert M == brute, (P, step, n, phase0)
                    else:
                        assert M == 0
                    got = rs.output_lengths([n], [step], [phase0])
                    assert got.tolist() == [M], (P, step, n, phase0, got)
                    assert rs.output_lengths([n], [step], [phase0], n_cols=7).tolist() == [min(M, 7)]
    assert rs.delay_items == Fraction(2 * 128 - 1, 4)


@pytest.mark.parametrize("Q,P", [(32, 12), (2, 1), (256, 16), (64, 3)])
def test_float32_restatement_keeps_the_bound(Q, P):
    n = 300
    x, h = _row(n, 5), _taps(Q, P)
    for step, phase0, freq in ((TWO32, 0, 0), (round(0.8929 * TWO32), TWO32 // 2, round(0.003 * TWO32)),
                               (round(2.2727 * TWO32), 3 * TWO32 + TWO32 // 4, -round(0.003 * TWO32)), (TWO32 + 1, 0, -(1 << 31)),
                               (1 << 28, 0, 12345)):
        y64 = ref.resample64(x, n, h, Q, step, phase0, freq, n_cols=600)
        y32 = ref.resample32(x, n, h, Q, step, phase0, freq, n_cols=600)
        bound = ref.error_bound(x, n, h, Q, step, phase0, n_cols=600)
        err = np.abs(y32.astype(np.complex128) - y64)
        assert np.all(err <= bound), float(np.max(err / np.maximum(bound, 1e-300)))
        assert np.all(y32[bound == 0] == 0)


def test_theta_against_python_integers():
    rng = np.random.default_rng(6)
    words = [0, 1, -1, round(0.003 * TWO32), -round(0.003 * TWO32), -(1 << 31), (1 << 31) - 1]
    words += [int(v) for v in rng.integers(-(1 << 31), 1 << 31, 40)]
    for freq in words:
        for pos in [0, 1, TWO32 - 1, TWO32, (5 << 32) + 0x80000000, (1 << 63) + 12345] + [int(v) for v in rng.integers(0, 1 << 62, 40)]:
            want = (freq * pos // TWO32) % TWO32  # floor of the exact product
            assert ref.theta(freq, pos) == want
            assert ref.theta_as_defined(freq, pos) == want, (freq, pos)


def test_taps_helper():
    pkg = ge.load_package()
    for Q, P in ((32, 12), (2, 1), (256, 16), (64, 3)):
        t = pkg.row_resampler_taps(Q, P)
        assert t.dtype == np.float32 and t.size == Q * P
        # kaiser_lowpass(Q P, Q, ...) with DC gain Q, rounded once: the Duc's prototype for an interpolation by Q
        assert np.array_equal(t, pkg.duc_taps(Q, P))
        assert np.max(np.abs(t - ref.kaiser_taps64(Q, P))) <= 1e-6 * Q
        assert abs(float(np.sum(t.astype(np.float64))) - Q) <= 1e-5 * Q
    # a decimating handle: the span grows with max_step, the edges shrink with it
    t = pkg.row_resampler_taps(32, 12, max_step=2.27)
    assert t.size == 32 * 28
    assert np.max(np.abs(t - ref.kaiser_taps64(32, 12, 2.27))) <= 1e-6 * 32
    assert np.array_equal(pkg.row_resampler_taps(32, 12, max_step=0.5), pkg.row_resampler_taps(32, 12))
    for bad in (dict(passband=0.5, stopband=0.25), dict(passband=-0.1), dict(passband=0.5, stopband=0.75),
                dict(passband=float("nan")), dict(phases=3), dict(phases=512), dict(phases=1), dict(taps_per_phase=0),
                dict(phases=256, taps_per_phase=17), dict(max_step=65.0), dict(max_step=0.001), dict(max_step=float("nan")),
                dict(phases=32, taps_per_phase=12, max_step=11.0)):
        with pytest.raises(pkg.Gr4pmError):
            pkg.row_resampler_taps(**bad)


def test_host_side_of_the_class():
    """what works without a GPU: the sizes' refusals, the steps of to_samples_per_symbol, the tile"""
    pkg = ge.load_package()
    for bad in (dict(phases=3), dict(phases=512), dict(phases=32, taps=np.ones(33, np.float32)),
                dict(phases=32, taps=np.ones(32 * 129, np.float32)), dict(phases=2, taps=np.array([1.0, np.inf], np.float32))):
        with pytest.raises(pkg.Gr4pmError):
            pkg.RowResampler(**bad)
    rs = pkg.RowResampler()
    assert (rs.phases, rs.taps_per_phase) == (32, 12)
    assert rs.steps_for([0.25, 0.28]) == [TWO32, round(Fraction(TWO32) / (4 * Fraction(0.28)))]
    for step in (1 << 26, TWO32, round(2.27 * TWO32), 1 << 38):
        T = rs.tile_items([step, 1 << 26])
        assert 1 <= T <= 1024 and (((T - 1) * step + TWO32 - 1) >> 32) + 12 <= 4096
    assert rs.tile_items([1 << 39]) == 0
    with pytest.raises(pkg.Gr4pmError):
        rs.output_lengths([10], [1 << 25])
    with pytest.raises(pkg.Gr4pmError):
        rs.output_lengths([10], [TWO32], [1 << 63])
    with pytest.raises(pkg.Gr4pmError):
        rs.output_lengths([TWO32], [TWO32])
