"""The Ddc's float64 references (tests/_ddc_ref.py) against each other, on the CPU: the definition (mix, filter, pick)
and the rotated-taps form the kernel implements; the grid-aligned setting against the Channelizer's reference; large
start indices against a direct evaluation with Python integers; the host-only tap design."""
import numpy as np
import pytest

import _channelizer_ref as cref
import _ddc_ref as dref

FREQS = [0.0, 0.5, -0.3137, 3.0 * 2.0 ** -32, 0.123456789, -0.05, 0.41, 1.0 / 3.0]


def stream(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def taps(L, seed):
    return np.random.default_rng(seed).standard_normal(L)


def scale(h, x):
    return np.sum(np.abs(h)) * np.max(np.abs(x))


def test_frequency_word():
    assert dref.frequency_word(0.0) == 0
    assert dref.frequency_word(0.5) == 1 << 31 and dref.quantised(0.5) == -0.5
    assert dref.frequency_word(-0.25) == 3 << 30 and dref.quantised(-0.25) == -0.25
    assert dref.frequency_word(3.0 * 2.0 ** -32) == 3
    assert dref.frequency_word(1.0) == 0 and dref.frequency_word(-7.0) == 0 and dref.frequency_word(1e300) == 0
    assert dref.frequency_word(2.5 * 2.0 ** -32) == 2 and dref.frequency_word(3.5 * 2.0 ** -32) == 4  # ties to even
    assert dref.frequency_word(-1e-30) == 0
    assert dref.frequency_word(5.25) == 1 << 30


@pytest.mark.parametrize("D,L,K", [(5, 60, 3), (1, 1, 1), (3, 7, 2)])
def test_definition_equals_rotated_taps_form(D, L, K):
    x = stream(40 * D + L + D // 2 + 3, D + L)
    h = taps(L, K)
    for start in (0, 12345):
        a = dref.ddc64(x, h, D, FREQS[:K], start)
        b = dref.ddc64_rotated(x, h, D, FREQS[:K], start, frames_per_block=7)
        assert a.shape == b.shape == (K, x.size // D)
        assert np.max(np.abs(a - b)) <= 1e-12 * scale(h, x)


def test_grid_aligned_setting_is_the_channelizer():
    M, P = 8, 5
    x = stream(60 * M + 3, 1)
    h = cref.kaiser_taps64(M, P) * M + 0.05 * taps(P * M, 2)
    want = cref.analysis64_polyphase(x, h, M)
    for fn in (dref.ddc64, dref.ddc64_rotated):
        got = fn(x, h, M, [k / M for k in range(M)])
        assert got.shape == want.shape
        assert np.max(np.abs(got - want)) <= 1e-12 * scale(h, x)


@pytest.mark.parametrize("start", [(1 << 32) - 100, (1 << 40) + 3])
def test_large_start_index_against_python_integers(start):
    D, L, K = 5, 60, 3
    x = stream(70 * D + 2, 7)   # crosses 2^32 for the first start
    h = taps(L, 8)
    items = [0, 1, 11, 12, 19, 20, 21, 40, 69]
    want = dref.ddc64_direct(x, h, D, FREQS[2:2 + K], start, items)
    for fn in (dref.ddc64, dref.ddc64_rotated):
        got = fn(x, h, D, FREQS[2:2 + K], start)[:, items]
        assert np.max(np.abs(got - want)) <= 1e-12 * scale(h, x)
    # the start matters: from 0 the same stream gives other values
    assert np.max(np.abs(dref.ddc64(x, h, D, FREQS[2:2 + K], 0)[:, items] - want)) > 1e-3 * scale(h, x)


def test_window_max():
    rng = np.random.default_rng(3)
    for D, L in [(5, 60), (1, 1), (3, 7), (20, 161), (16, 100)]:
        x = rng.standard_normal(37 * D + 4) * (rng.random(37 * D + 4) < 0.2)
        got = dref.window_max(x, D, L)
        for n in range(x.size // D):
            i = n * D + D - 1
            assert got[n] == np.max(np.abs(x[max(0, i - L + 1):i + 1]))


def test_tap_design():
    """gr4pm_ddc_taps (host only): the stated Kaiser design for any decimation, the channelizer's floats for a
    power-of-two one, and the refusals"""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    for D, P in [(5, 12), (20, 8), (3, 32), (1000, 2), (1, 1), (1, 12), (7, 1)]:
        h = pkg.ddc_taps(D, P)
        assert h.dtype == np.float32 and h.size == D * P
        h64 = dref.kaiser_taps64(D, D * P)
        assert np.all(np.abs(h - h64) <= dref.EPS32 * np.abs(h64) + 1e-12)  # one rounding to float32
        assert abs(float(np.sum(h.astype(np.float64))) - 1.0) < 1e-6
    for M, P in [(2, 1), (16, 12), (64, 12), (1024, 3)]:
        assert np.array_equal(pkg.ddc_taps(M, P).view(np.uint32), pkg.channelizer_taps(M, P).view(np.uint32))
    assert np.array_equal(pkg.ddc_taps(16, 12, 0.2, 0.6).view(np.uint32), pkg.channelizer_taps(16, 12, 0.2, 0.6).view(np.uint32))
    for bad in [(0, 12), (1025, 1), (5, 0), (1024, 9)]:
        with pytest.raises(pkg.Gr4pmError):
            pkg.ddc_taps(*bad)
    with pytest.raises(pkg.Gr4pmError):
        pkg.ddc_taps(5, 12, 0.75, 0.25)
