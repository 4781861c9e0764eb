"""The rational Ddc's float64 references (tests/_ddc_rational_ref.py) against each other, on the CPU: the definition
(mix, zero-stuff, filter, pick) and the rotated-taps form the kernel implements, large start indices against a direct
evaluation with Python integers, I = 1 against the integer Ddc's reference, the item count, and the host-only tap
design."""
import numpy as np
import pytest

import _ddc_rational_ref as rref
import _ddc_ref as dref

FREQS = [0.0, 0.5, -0.3137, 3.0 * 2.0 ** -32, 0.123456789, -0.05, 0.41, 1.0 / 3.0]


def stream(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def taps(L, seed):
    return np.random.default_rng(seed).standard_normal(L)


def scale(h, x):
    return np.sum(np.abs(h)) * np.max(np.abs(x))


@pytest.mark.parametrize("I,D,L,K", [(4, 25, 300, 3), (3, 2, 24, 1), (5, 12, 61, 2), (7, 1, 30, 1), (2, 3, 1, 1),
                                     (64, 5, 7, 2)])
@pytest.mark.parametrize("start", [0, 12345, (1 << 32) - 1000, (1 << 40) + 3])
def test_rotated_form_equals_the_definition_and_the_direct_sums(I, D, L, K, start):
    n = 1200 if D <= 5 else 50 * D + L // I + D // 2 + 3  # the first large start crosses 2^32 after 1000 samples
    x = stream(n, I + D + L)
    h = taps(L, K)
    a = rref.rddc64(x, h, I, D, FREQS[:K], start)
    b = rref.rddc64_rotated(x, h, I, D, FREQS[:K], start, items_per_block=7)
    assert a.shape == b.shape == (K, n * I // D)
    assert np.max(np.abs(a - b)) <= 1e-12 * scale(h, x)
    F = a.shape[1]
    which = sorted({0, 1, I - 1, I, F // 2, F - 2, F - 1} & set(range(F)))
    c = rref.rddc64_direct(x, h, I, D, FREQS[:K], start, which)
    assert np.max(np.abs(b[:, which] - c)) <= 1e-12 * scale(h, x)
    if start and K >= 3:  # the start matters (to a channel whose frequency is neither 0 nor 0.5)
        assert np.max(np.abs(rref.rddc64(x, h, I, D, FREQS[:K], 0) - a)) > 1e-3 * scale(h, x)


@pytest.mark.parametrize("D,L,K", [(5, 60, 3), (1, 1, 1), (3, 7, 2)])
def test_interpolation_one_is_the_integer_ddc(D, L, K):
    x = stream(40 * D + L + D // 2 + 3, D + L)
    h = taps(L, K)
    want = dref.ddc64(x, h, D, FREQS[:K], 777)
    for fn in (rref.rddc64, rref.rddc64_rotated):
        got = fn(x, h, 1, D, FREQS[:K], 777)
        assert got.shape == want.shape
        assert np.max(np.abs(got - want)) <= 1e-12 * scale(h, x)


def test_every_branch_is_an_integer_ddc():
    """items n_p + I j of branch p: the integer-D Ddc with the taps h[p::I] on the stream delayed so that its frames
    end where the branch's items do"""
    I, D, L = 5, 12, 61
    x, h = stream(40 * D + 3, 3), taps(L, 4)
    y = rref.rddc64(x, h, I, D, FREQS[2:4])
    j, p = rref.items(x.size, I, D)
    for b in range(I):
        idx = np.nonzero(p == b)[0]
        z = (D - 1 - int(j[idx[0]])) % D
        yi = dref.ddc64(np.concatenate([np.zeros(z), x]), h[b::I], D, FREQS[2:4], start=-z % (1 << 32))
        assert np.all(np.diff(j[idx]) == D)
        n_int = (j[idx] + z - D + 1) // D
        assert np.max(np.abs(y[:, idx] - yi[:, n_int])) <= 1e-12 * scale(h, x)


@pytest.mark.parametrize("I,D", [(4, 25), (3, 2), (5, 12), (7, 1), (64, 1023), (1, 5)])
def test_item_count_is_floor_n_i_over_d(I, D):
    """item n exists as soon as its sample has arrived: its input index is below N exactly when n < floor(N I / D)"""
    for N in list(range(0, 300)) + [2 * D, 2 * D + 1, 3 * D - 1]:
        j, p = rref.items(N, I, D)
        assert j.size == N * I // D
        assert j.size == 0 or j[-1] < N
        m_next = j.size * D + D - 1
        assert m_next // I >= N
        assert np.all(p == (np.arange(j.size) * D + D - 1) % I)
        assert rref.rddc64(np.ones(N), np.ones(3), I, D, [0.0]).shape == (1, N * I // D)


def test_window_max_and_branch_sums():
    rng = np.random.default_rng(3)
    for I, D, L in [(4, 25, 300), (3, 2, 24), (5, 12, 61), (7, 1, 30)]:
        N = 37 * D + 4
        x = rng.standard_normal(N) * (rng.random(N) < 0.2)
        j, _ = rref.items(N, I, D)
        P = -(-L // I)
        got = rref.window_max(x, j, P)
        for n in range(j.size):
            assert got[n] == np.max(np.abs(x[max(0, j[n] - P + 1):j[n] + 1]))
        h = rng.standard_normal(L)
        s = rref.branch_abs_sum(h, I)
        assert s.shape == (I,) and all(abs(s[b] - np.sum(np.abs(h[b::I]))) < 1e-12 for b in range(I))


def test_tap_design():
    """gr4pm_ddc_rational_taps (host only): the stated Kaiser design with DC gain I, the floats of gr4pm_ddc_taps at
    I = 1, and the refusals, the cutoff's among them"""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    for I, D, P in [(4, 25, 12), (5, 12, 12), (3, 50, 8), (64, 1023, 8), (63, 64, 12), (2, 3, 1), (4, 25, 1)]:
        h = pkg.ddc_rational_taps(I, D, P)
        assert h.dtype == np.float32 and h.size == D * P
        h64 = rref.rational_taps64(I, D, D * P)
        assert np.all(np.abs(h - h64) <= dref.EPS32 * np.abs(h64) + 1e-12)  # one rounding to float32, after the gain
        assert abs(float(np.sum(h.astype(np.float64))) - I) < 1e-5 * I
        if P >= 8:  # every branch has gain about 1
            assert np.all(np.abs(rref.branch_taps(h, I).sum(axis=1) - 1.0) < 1e-3)
    # band edges in units of the output rate, I > D: the cutoff up to half of the INPUT rate, D / I of the output's
    h = pkg.ddc_rational_taps(3, 2, 12, 0.25 * 2 / 3, 0.75 * 2 / 3)
    h64 = rref.rational_taps64(3, 2, 24, 0.25 * 2 / 3, 0.75 * 2 / 3)
    assert np.all(np.abs(h - h64) <= dref.EPS32 * np.abs(h64) + 1e-12)
    for D, P in [(5, 12), (20, 8), (1000, 2), (1, 12), (16, 12)]:
        assert np.array_equal(pkg.ddc_rational_taps(1, D, P).view(np.uint32), pkg.ddc_taps(D, P).view(np.uint32))
    assert np.array_equal(pkg.ddc_rational_taps(1, 16, 12, 0.2, 0.6).view(np.uint32), pkg.ddc_taps(16, 12, 0.2, 0.6).view(np.uint32))
    for bad in [(0, 5, 12), (65, 5, 12), (4, 0, 12), (4, 1025, 1), (4, 25, 0), (4, 1023, 9)]:
        with pytest.raises(pkg.Gr4pmError):
            pkg.ddc_rational_taps(*bad)
    with pytest.raises(pkg.Gr4pmError):
        pkg.ddc_rational_taps(4, 25, 12, 0.75, 0.25)
    # the cutoff: at most half of the output rate (D >= I) ...
    assert pkg.ddc_rational_taps(4, 25, 12, 0.25, 0.75).size == 300
    with pytest.raises(pkg.Gr4pmError, match="cutoff"):
        pkg.ddc_rational_taps(4, 25, 12, 0.25, 0.76)
    # ... and at most half of the input rate (I > D): the defaults are beyond it
    with pytest.raises(pkg.Gr4pmError, match="cutoff"):
        pkg.ddc_rational_taps(3, 2, 12)
    with pytest.raises(pkg.Gr4pmError, match="cutoff"):
        pkg.ddc_rational_taps(3, 2, 12, 0.2, 0.47)
    assert pkg.ddc_rational_taps(3, 2, 12, 0.2, 0.46).size == 24
