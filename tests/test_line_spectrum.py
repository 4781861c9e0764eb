"""The LineSpectrum block on the GPU against the float64 restatement of its definition (tests/_line_spectrum_ref.py) within
the derived bound stated there, and its exact properties: rows with lengths that are never read beyond, a row's bits that
depend on that row alone, the envelope's symmetry, the bin layout, power-of-two gains, strides, refusals.

Rows: R = 6 with the lengths (0, 1, 2047, 2049, 5000, 40000) of n_cols = 40000 items, so the last row ends where the
allocation ends.  S = 0, 1, 1 segments for the first three."""
import ctypes as C
import functools

import numpy as np
import pytest

import _line_spectrum_ref as lref
from _frontend import bits, dev, host, load_package

pytestmark = pytest.mark.gpu

N = lref.N
LENGTHS = (0, 1, 2047, 2049, 5000, 40000)
N_COLS = 40000
HOPS = (2048, 1024, 1000, 256)
GAINS = np.array([1.0, 0.75, 1.25, 0.8125, 1.0, 0.5], dtype=np.float32)


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@functools.lru_cache(maxsize=None)
def stimulus(rows=6, seed=11):
    """seeded Gaussian noise plus two tones per row, one of them off the bin grid"""
    rng = np.random.default_rng(seed)
    t = np.arange(N_COLS, dtype=np.float64)
    x = 0.5 * (rng.standard_normal((rows, N_COLS)) + 1j * rng.standard_normal((rows, N_COLS)))
    for r in range(rows):
        x[r] += 0.8 * np.exp(2j * np.pi * (0.012345 + 0.001 * r) * t) + 0.3 * np.exp(2j * np.pi * (-77.0 / 2048) * t)
    x = x.astype(np.complex64)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(statistic, hop):
    """the float64 rows and their bounds, computed once per (statistic, hop)"""
    x, w = stimulus(), lref.hann()
    return [lref.row_spectrum(x[r], LENGTHS[r], hop, w, statistic, GAINS[r]) for r in range(len(LENGTHS))]


def raw(pkg, ls, x, lengths, statistic, gains=None):
    """gr4pm_line_spectrum_process through ctypes on a device array x[R, n]; gains: numpy float32 or None"""
    import torch
    R, n = x.shape
    out = torch.full((R, N), float("nan"), dtype=torch.float64, device="cuda")
    ln = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.uint64)
    g = None if gains is None else dev(np.ascontiguousarray(gains, dtype=np.float32))
    pkg._abi.check(pkg.lib().gr4pm_line_spectrum_process(
        ls._h, x.data_ptr(), x.stride(0) if R > 1 else n, n, None if ln is None else ln.ctypes.data_as(C.c_void_p), R,
        None if g is None else g.data_ptr(), pkg._abi.LINE_STATISTICS[statistic], out.data_ptr()), "line_spectrum")
    return host(out)


@pytest.mark.parametrize("statistic", lref.STATISTICS)
@pytest.mark.parametrize("hop", HOPS)
def test_within_the_float64_bound(pkg, statistic, hop):
    got = raw(pkg, pkg.LineSpectrum(hop=hop), dev(stimulus()), LENGTHS, statistic, GAINS)
    worst = 0.0
    for r, ref in enumerate(reference(statistic, hop)):
        if ref["segments"] == 0:
            assert not got[r].any()
            continue
        err = np.abs(got[r] - ref["out"]) * (ref["segments"] * ref["window_power"])
        worst = max(worst, lref.worst_ratio(err, ref["bound"]))
        assert np.all(err <= ref["bound"]), (r, lref.worst_ratio(err, ref["bound"]))
    print(f"{statistic} hop {hop}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("statistic", lref.STATISTICS)
def test_nothing_behind_a_rows_length_is_read(pkg, statistic):
    """NaN behind the lengths 1 and 2047 (and everything of the empty row): the result is finite and has the bits of the
    zero-padded rows'"""
    x = stimulus()[:3].copy()
    ls = pkg.LineSpectrum(hop=1024)
    padded = x.copy()
    for r in range(3):
        padded[r, LENGTHS[r]:] = 0
        x[r, LENGTHS[r]:] = np.nan + 1j * np.nan
    want = raw(pkg, ls, dev(padded), LENGTHS[:3], statistic, GAINS[:3])
    got = raw(pkg, ls, dev(x), LENGTHS[:3], statistic, GAINS[:3])
    assert np.isfinite(got).all()
    assert not got[0].any() and got[2].any()  # (one item under the Hann window, whose w[0] is 0, gives zeros too)
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("statistic", lref.STATISTICS)
@pytest.mark.parametrize("hop", [1024, 256])
def test_a_row_depends_on_that_row_alone(pkg, statistic, hop):
    ls, d = pkg.LineSpectrum(hop=hop), dev(stimulus())
    both = raw(pkg, ls, d, LENGTHS, statistic, GAINS)
    assert np.array_equal(bits(raw(pkg, ls, d, LENGTHS, statistic, GAINS)), bits(both))  # the same call twice
    for r in range(len(LENGTHS)):
        alone = raw(pkg, ls, d[r:r + 1], LENGTHS[r:r + 1], statistic, GAINS[r:r + 1])
        assert np.array_equal(bits(alone[0]), bits(both[r])), r


def test_seventy_rows_equal_their_split(pkg):
    """the class cuts 70 rows into calls of 64 and 6; the rows equal those of calls of their own"""
    import torch
    rng = np.random.default_rng(2)
    x = (rng.standard_normal((70, 3000)) + 1j * rng.standard_normal((70, 3000))).astype(np.complex64)
    lengths = rng.integers(0, 3001, 70)
    lengths[:3] = (0, 3000, 2048)
    ls, d = pkg.LineSpectrum(hop=500), dev(x)
    for statistic in lref.STATISTICS:
        whole = host(ls.process_rows(d, lengths, statistic))
        first = host(ls.process_rows(d[:64], lengths[:64], statistic))
        last = host(ls.process_rows(d[64:], lengths[64:], statistic))
        assert whole.shape == (70, N) and np.isfinite(whole).all()
        assert np.array_equal(bits(whole), bits(np.concatenate([first, last])))
        gains = 1.0 / np.sqrt([np.mean(np.abs(x[r, :lengths[r]].astype(np.complex128)) ** 2) if lengths[r] else 1.0
                               for r in (1, 5)])
        for i, r in enumerate((1, 5)):  # normalize=True is a gain of 1 / rms over the row's length
            ref = lref.row_spectrum(x[r], int(lengths[r]), 500, lref.hann(), statistic, np.float32(gains[i]))
            assert np.allclose(whole[r], ref["out"], rtol=1e-4, atol=1e-6 * ref["out"].max())
    assert ls.process_rows(d[:0], None).shape == (0, N)
    assert ls.process_rows(d, None, "envelope", normalize=False).dtype == torch.float64


@pytest.mark.parametrize("k0", [0, 1, 63, 64, 511, 512])
def test_layout_one_tone_at_a_bin_centre(pkg, k0):
    x = np.exp(2j * np.pi * k0 * np.arange(3 * N) / N).astype(np.complex64)[None, :]
    ls = pkg.LineSpectrum(hop=2048, window=np.ones(N, dtype=np.float32))
    fourth, square = raw(pkg, ls, dev(x), None, "fourth")[0], raw(pkg, ls, dev(x), None, "square")[0]
    for sp, k in ((fourth, (4 * k0) % N), (square, (2 * k0) % N)):
        assert int(np.argmax(sp)) == k
        assert abs(sp[k] - N) < 1e-3 * N  # |Y[k]|^2 / sum w^2 = N^2 / N
        assert np.sum(sp) - sp[k] < 1e-5 * N


@pytest.mark.parametrize("hop", HOPS)
def test_the_envelope_is_bit_symmetric(pkg, hop):
    got = raw(pkg, pkg.LineSpectrum(hop=hop), dev(stimulus()), LENGTHS, "envelope", GAINS)
    assert np.array_equal(bits(got), bits(got[:, (N - np.arange(N)) % N]))
    assert got[3:].all()


# out scales with gain^(2 deg), deg the degree of y in u: |u|^2 and u^2 have 2, u^4 has 4
GAIN_EXPONENT = {"envelope": 4, "square": 4, "fourth": 8}


@pytest.mark.parametrize("statistic", lref.STATISTICS)
def test_power_of_two_gains_are_exact(pkg, statistic):
    ls, d = pkg.LineSpectrum(hop=1000), dev(stimulus())
    base = raw(pkg, ls, d, LENGTHS, statistic, None)
    assert np.array_equal(bits(base), bits(raw(pkg, ls, d, LENGTHS, statistic, np.ones(6, dtype=np.float32))))
    for e in (5, -5):
        got = raw(pkg, ls, d, LENGTHS, statistic, np.full(6, 2.0 ** e, dtype=np.float32))
        assert np.array_equal(got, base * 2.0 ** (e * GAIN_EXPONENT[statistic]))


def test_no_lengths_means_full_rows_and_strides_work(pkg):
    import torch
    x = stimulus()[:, :5000]
    ls = pkg.LineSpectrum(hop=1024)
    d = dev(x)
    full = raw(pkg, ls, d, None, "fourth")
    assert np.array_equal(bits(full), bits(raw(pkg, ls, d, [5000] * 6, "fourth")))
    wide = torch.full((6, 5000 + 37), float("nan"), dtype=torch.complex64, device="cuda")
    wide[:, :5000] = d
    view = wide[:, :5000]
    assert view.stride(0) == 5037
    assert np.array_equal(bits(raw(pkg, ls, view, None, "fourth")), bits(full))
    for statistic in lref.STATISTICS:
        assert np.array_equal(bits(host(ls.process_rows(view, None, statistic, normalize=False))),
                              bits(host(ls.process_rows(d, None, statistic, normalize=False))))


def test_refusals(pkg):
    import torch
    lib, abi = pkg.lib(), pkg._abi
    h = C.c_void_p()
    for fft_size, hop, window in [(1024, 512, None), (2048, 0, None), (2048, 2049, None),
                                  (2048, 1024, np.full(N, np.inf, dtype=np.float32))]:
        p = abi.LineSpectrumParams(fft_size, hop, None if window is None else window.ctypes.data_as(C.c_void_p), None)
        assert lib.gr4pm_line_spectrum_create(C.byref(p), C.byref(h)) == -1 and not h.value
        assert lib.gr4pm_last_error()
    for kw in [dict(fft_size=1024), dict(hop=0), dict(hop=2049), dict(window=np.ones(5)),
               dict(window=np.full(N, np.nan, dtype=np.float32))]:
        with pytest.raises(pkg.Gr4pmError):
            pkg.LineSpectrum(**kw)
    ls = pkg.LineSpectrum()
    x = dev(stimulus()[:, :4096])
    out = torch.zeros((65, N), dtype=torch.float64, device="cuda")
    ln = (C.c_uint64 * 65)(*([4096] * 65))

    def call(xp, stride, n_cols, lengths, rows, stat, outp):
        return lib.gr4pm_line_spectrum_process(ls._h, xp, stride, n_cols, lengths, rows, None, stat, outp)

    assert call(x.data_ptr(), 4096, 4096, ln, 65, 2, out.data_ptr()) == -1       # R > 64
    assert b"64" in lib.gr4pm_last_error()
    ln[1] = 4097
    assert call(x.data_ptr(), 4096, 4096, ln, 6, 2, out.data_ptr()) == -1        # n_r > n_cols
    ln[1] = 4096
    assert call(x.data_ptr(), 4095, 4096, ln, 6, 2, out.data_ptr()) == -1        # R > 1 with stride < n_cols
    assert call(x.data_ptr(), 4095, 4096, ln, 1, 2, out.data_ptr()) == 0         # one row: the stride does not matter
    for stat in (-1, 3):
        assert call(x.data_ptr(), 4096, 4096, ln, 6, stat, out.data_ptr()) == -1  # an unknown statistic
    assert call(None, 4096, 4096, ln, 6, 2, out.data_ptr()) == -1                # no x, lengths not zero
    zero = (C.c_uint64 * 6)(*([0] * 6))
    out.fill_(1.0)
    assert call(None, 4096, 4096, zero, 6, 2, out.data_ptr()) == 0               # no x, nothing to read
    assert not host(out[:6]).any()
    assert call(x.data_ptr(), 4096, 4096, ln, 6, 2, None) == -1                  # no out
    assert call(x.data_ptr(), 4096, 4096, ln, 0, 2, None) == 0                   # R = 0: nothing done
    torch.cuda.synchronize()
    with pytest.raises(pkg.Gr4pmError):
        ls.process_rows(x, None, "cube")
    with pytest.raises(pkg.Gr4pmError):
        ls.process_rows(x, [4097] * 6)
    with pytest.raises(pkg.Gr4pmError):
        ls.process_rows(x, [1, 2])
    with pytest.raises(TypeError):
        ls.process_rows(x[0])
    for kw in [dict(order=3), dict(max_offset=0.125), dict(max_offset=0.0)]:
        with pytest.raises(pkg.Gr4pmError):
            ls.carrier_offset(x, **kw)
    for kw in [dict(min_rate=0.0), dict(max_rate=0.5), dict(min_rate=0.3, max_rate=0.2)]:
        with pytest.raises(pkg.Gr4pmError):
            ls.symbol_rate(x, **kw)


def test_offset_and_rate_of_synthetic_rows(pkg):
    """a QPSK row with a known offset and a known symbol rate, noiseless: the two estimators through the class"""
    rng = np.random.default_rng(4)
    sps, n_sym, delta = 4, 1500, 0.0123
    sym = np.exp(0.5j * np.pi * rng.integers(0, 4, n_sym) + 0.25j * np.pi)
    up = np.zeros(n_sym * sps, dtype=np.complex128)
    up[::sps] = sym
    t = np.arange(-32, 33) / sps  # raised-cosine-like smooth pulse with excess bandwidth: a Hann-tapered sinc
    pulse = np.sinc(t) * np.cos(0.35 * np.pi * t) / (1.0 - (0.7 * t) ** 2 + 1e-12)
    x = np.convolve(up, pulse)[: n_sym * sps] * np.exp(2j * np.pi * delta * np.arange(n_sym * sps))
    d = dev(x.astype(np.complex64)[None, :])
    ls = pkg.LineSpectrum()
    off = ls.carrier_offset(d)
    assert abs(off["offset"][0] - delta) < 1.0 / (4 * N) and off["margin_db"][0] >= 6
    rate = ls.symbol_rate(d)
    assert abs(rate["rate"][0] - 1.0 / sps) < 1e-3 / sps and rate["snr_db"][0] > 0
