"""The Spectrogram block on the GPU against the float64 restatement of its definition (tests/_spectrogram_ref.py) within a
derived bound, and its exact properties: rows do not depend on how the stream is cut into calls, R = 1 has no detector,
rows are where their time is, the lane / register to bin layout, power-of-two scaling, short streams, integer ingest,
rows_cap, refusals, and the band power.

The bound (tests/_spectrogram_ref.py: bound).  With X64_s the float64 transform of segment s and delta_s = 8 * 2^-24 *
||X64_s||_2 (C = 8 is what tests/test_syncword_float64.py holds every GPU form of this transform to), per row and bin,
divided by the row's normaliser (R sum w^2 for the mean, sum w^2 for the maximum)
    mean: sum_s (2 |X64_s| delta_s + delta_s^2) + R * 2^-24 * sum_s |X64_s|^2
    max:  max_s (2 |X64_s| delta_s + delta_s^2)
plus 3 * 2^-24 * row64 for the rounding of inv and of the one product at the store.  First order, worst case: not a fit.
tests/test_spectrogram_ref.py holds a float32 numpy transform to the same bound at the same shapes."""
import ctypes as C

import numpy as np
import pytest

import _spectrogram_ref as gref
from _frontend import dev, exact_iq_forms, host, load_package

pytestmark = pytest.mark.gpu

N = 2048
CUTS = (1, 63, 2048, 4097)
ERR_INVALID, ERR_OVERFLOW = -1, -5


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run(pkg, x, hop, R=1, detector="mean", kind="hann", cuts=(), scale=None, sg=None):
    """x (numpy complex64, or integer IQ [n, 2]) through a Spectrogram in calls of the lengths `cuts`, then the rest; the
    rows of all calls joined, on the host.  Every call returns exactly the rows gr4pm_spectrogram_rows announced."""
    import torch
    sg = sg or pkg.Spectrogram(hop=hop, average=R, detector=detector, window=None if kind == "hann" else np.ones(N, dtype=np.float32))
    d, lo, parts = dev(x), 0, []

    def call(piece):
        want = sg.rows(piece.shape[0])
        out = sg.process_bulk(piece, scale=scale) if scale is not None else sg.process_bulk(piece)
        assert out.dtype == torch.float32 and tuple(out.shape) == (want, N)
        parts.append(out)

    for c in cuts:
        call(d[lo:lo + c])
        lo = min(lo + c, len(x))
    if lo < len(x) or not cuts:
        call(d[lo:])
    rows = host(torch.cat(parts, dim=0))
    assert sg.rows_done == rows.shape[0]
    return rows


@pytest.mark.parametrize("detector", gref.DETECTORS)
@pytest.mark.parametrize("kind", gref.KINDS)
@pytest.mark.parametrize("hop,n,R", gref.SHAPES)
def test_within_the_float64_bound(pkg, hop, n, R, kind, detector):
    got = run(pkg, gref.stimulus(n), hop, R, detector, kind)
    assert got.shape == (gref.n_rows(n, hop, R), N)
    worst = gref.worst_over_bound(got, n, hop, R, detector, kind)
    print(f"hop {hop} n {n} R {R} {kind} {detector}: {got.shape[0]} rows, worst error / bound {worst:.3f}")
    assert worst <= 1.0


def test_white_noise_reads_its_power(pkg):
    """sigma^2 = 0.5 in every bin of a mean row, within the spread of 12 rows of 3 segments"""
    rng = np.random.default_rng(1)
    x = (0.5 * (rng.standard_normal(40000) + 1j * rng.standard_normal(40000))).astype(np.complex64)
    rows = run(pkg, x, 1000, 3)
    assert rows.shape == (12, N) and abs(float(np.mean(rows)) - 0.5) < 0.02


@pytest.mark.parametrize("detector", gref.DETECTORS)
@pytest.mark.parametrize("hop,R", [(1024, 3), (1000, 3), (1, 64)])
def test_cuts_do_not_exist(pkg, hop, R, detector):
    """the carried samples, the carried row and the hand-out of rows to waves: the rows of five calls are the rows of one,
    bit for bit"""
    n = 2048 + 8191 if hop == 1 else 40000
    x = gref.stimulus(n)
    whole = run(pkg, x, hop, R, detector)
    cut = run(pkg, x, hop, R, detector, cuts=CUTS)
    assert whole.shape == cut.shape == (gref.n_rows(n, hop, R), N) and whole.shape[0] >= 12
    assert np.array_equal(bits(cut), bits(whole))
    # calls that end inside a row over and over: one sample at a time across two rows' worth of segments at hop 1
    if hop == 1:
        m = 2048 + 2 * R
        single = run(pkg, x[:m], hop, R, detector, cuts=(2040,) + (1,) * (m - 2040))
        assert single.shape == (2, N) and np.array_equal(bits(single), bits(whole[:2]))


def test_average_one_has_no_detector(pkg):
    x = gref.stimulus(40000)
    mean, mx = run(pkg, x, 1000, 1, "mean"), run(pkg, x, 1000, 1, "max")
    assert mean.shape == (38, N) and np.array_equal(bits(mean), bits(mx))


@pytest.mark.parametrize("hop,R,n,rows_that_hold", [(1, 1, 2048 + 8191, {0: 1, 4100: 2048, 2048 + 8190: 1}),
                                                   (1000, 3, 40000, {0: 1, 4100: 1, 39999: 0})])
def test_rows_are_where_their_time_is(pkg, hop, R, n, rows_that_hold):
    """zeros with a single 1.0 at sample m under the rectangular window: the rows whose samples [t R hop, t R hop + (R - 1)
    hop + N) hold m are nonzero in every bin, all other rows are exactly 0.0"""
    adv, span = R * hop, (R - 1) * hop + N
    assert sorted(rows_that_hold) == [0, 4100, n - 1]
    for m, count in rows_that_hold.items():
        x = np.zeros(n, dtype=np.complex64)
        x[m] = 1.0
        for detector in gref.DETECTORS:
            rows = run(pkg, x, hop, R, detector, "rect")
            assert rows.shape[0] == gref.n_rows(n, hop, R)
            t = np.arange(rows.shape[0])
            holds = (t * adv <= m) & (m < t * adv + span)
            assert holds.sum() == count
            assert np.all(rows[holds] != 0.0), (m, detector)
            assert not rows[~holds].any(), (m, detector)
    sg = pkg.Spectrogram(hop=hop, average=R)
    assert (sg.row_advance, sg.row_span) == (adv, span)


def test_layout_one_tone_at_a_bin_centre(pkg):
    """k0 on both sides of every boundary between two rows of 64 bins: the peak of every row is at k0, N high"""
    sg = pkg.Spectrogram(hop=2048, window=np.ones(N, dtype=np.float32))
    for j in range(32):
        for k0 in ((64 * j - 1) % N, 64 * j):
            x = np.exp(2j * np.pi * k0 * np.arange(3 * N) / N).astype(np.complex64)
            sg.reset()
            rows = run(pkg, x, 2048, sg=sg)
            assert rows.shape == (3, N)
            assert np.all(np.argmax(rows, axis=1) == k0), k0
            assert np.all(np.abs(rows[:, k0] - N) < 1e-3 * N)  # |X[k0]|^2 / sum w^2 = N^2 / N
            assert np.all(rows.sum(axis=1) - rows[:, k0] < 1e-6 * N)


@pytest.mark.parametrize("detector", gref.DETECTORS)
def test_power_of_two_scaling_is_exact(pkg, detector):
    x = gref.stimulus(40000)
    base = run(pkg, x, 1000, 3, detector)
    for e in (10, -10):
        rows = run(pkg, (x * np.float32(2.0 ** e)).astype(np.complex64), 1000, 3, detector)
        assert np.array_equal(bits(rows), bits(base * np.float32(4.0 ** e)))


def test_short_streams(pkg):
    x = gref.stimulus(40000)[:4096]
    d = dev(x)
    sg = pkg.Spectrogram(hop=2048, average=2)
    assert sg.rows(4095) == 0 and sg.rows(4096) == 1
    assert tuple(sg.process_bulk(d[:0]).shape) == (0, N)  # a zero-length call is fine
    assert tuple(sg.process_bulk(d[:4095]).shape) == (0, N) and sg.rows_done == 0
    assert sg.rows(0) == 0 and sg.rows(1) == 1
    row = sg.process_bulk(d[4095:])  # the 4096th sample, in a call of its own
    assert tuple(row.shape) == (1, N) and sg.rows_done == 1
    want = gref.rows(x, 2048, 2, "mean", gref.window_of("hann"))
    err = np.abs(host(row).astype(np.float64) - want)
    assert np.all(err <= gref.bound(gref.sref.spectra(x, 2048, gref.window_of("hann")), 2, "mean", gref.window_of("hann")))
    assert np.array_equal(sg.frequencies, np.where(np.arange(N) < N // 2, np.arange(N), np.arange(N) - N) / N)


@pytest.mark.parametrize("form", [1, 2, 3], ids=["sc16", "sc8", "cu8"])
def test_integer_iq_equals_unpacked(pkg, form):
    _, forms = exact_iq_forms(20000, seed=3)
    v, _ = forms[form]
    for scale in (forms[form][1], 0.0123):  # the exact scale (None: the format's default), and one that makes the unpack round
        unpacked = host(pkg.iq_unpack(dev(v), scale=scale))
        for detector in gref.DETECTORS:
            got = run(pkg, v, 1000, 3, detector, cuts=CUTS, scale=scale)
            want = run(pkg, unpacked, 1000, 3, detector, cuts=CUTS)
            assert got.shape == (gref.n_rows(20000, 1000, 3), N) and np.array_equal(bits(got), bits(want))


def test_formats_mix_on_one_handle(pkg):
    import torch
    x, forms = exact_iq_forms(20000, seed=4)
    want = run(pkg, x, 1000, 3)
    sg = pkg.Spectrogram(hop=1000, average=3)
    devs = [(dev(v), s) for v, s in forms]
    lo, parts = 0, []
    for i, c in enumerate(CUTS + (3000, 500, 20000)):
        v, s = devs[i % 4]
        parts.append(sg.process_bulk(v[lo:lo + c], scale=s) if s is not None else sg.process_bulk(v[lo:lo + c]))
        lo = min(lo + c, 20000)
    assert np.array_equal(bits(host(torch.cat(parts, dim=0))), bits(want))


def test_rows_cap_one_too_small(pkg):
    """GR4PM_ERR_OVERFLOW, and the handle is as it was: the same call with enough room then gives the rows an untouched
    handle gives"""
    import torch
    L = pkg.lib()
    x = gref.stimulus(40000)
    d = dev(x)
    want = run(pkg, x, 1000, 3)
    sg = pkg.Spectrogram(hop=1000, average=3)
    first = sg.process_bulk(d[:6000])  # four segments: a row, and a carried row and carried samples in the handle
    assert first.shape[0] == 1
    rows = sg.rows(34000)
    assert rows == 11
    out = torch.full((rows, N), -1.0, dtype=torch.float32, device="cuda")
    got = C.c_size_t(77)
    assert L.gr4pm_spectrogram_process(sg._h, d[6000:].data_ptr(), 34000, out.data_ptr(), rows - 1, C.byref(got)) == ERR_OVERFLOW
    assert got.value == 0 and sg.rows(34000) == rows
    assert L.gr4pm_spectrogram_process(sg._h, d[6000:].data_ptr(), 34000, out.data_ptr(), rows, C.byref(got)) == 0
    assert got.value == rows
    assert np.array_equal(bits(np.concatenate([host(first), host(out)])), bits(want))
    # the integer entry (format 1: GR4PM_IQ_SC16) refuses the same way
    v = dev(exact_iq_forms(5000, seed=1)[1][1][0])
    sg = pkg.Spectrogram(hop=1000)
    assert L.gr4pm_spectrogram_process_iq(sg._h, v.data_ptr(), 1, 0.0, 5000, out.data_ptr(), 2, C.byref(got)) == ERR_OVERFLOW
    assert sg.rows(5000) == 3


def test_refusals_and_reset(pkg):
    from gr4_packet_modem_amd import _abi
    L = pkg.lib()
    nan_window = np.ones(N, dtype=np.float32)
    nan_window[1500] = np.nan
    inf_window = np.ones(N, dtype=np.float32)
    inf_window[0] = np.inf
    for fft_size, hop, average, detector, window in (
            (2048, 0, 1, 0, None), (2048, 2049, 1, 0, None), (1024, 512, 1, 0, None), (4096, 1024, 1, 0, None),
            (2048, 1024, 1, 0, nan_window), (2048, 1024, 1, 0, inf_window), (2048, 1024, 0, 0, None), (2048, 1024, 65, 0, None),
            (2048, 1024, 1, 2, None), (2048, 1024, 1, 0xFFFFFFFF, None)):
        h = C.c_void_p(0x1234)
        p = _abi.SpectrogramParams(fft_size, hop, average, detector, None if window is None else window.ctypes.data_as(C.c_void_p), None)
        assert L.gr4pm_spectrogram_create(C.byref(p), C.byref(h)) == ERR_INVALID, (fft_size, hop, average, detector)
        assert h.value is None
    for kw in (dict(hop=0), dict(hop=2049), dict(fft_size=1024), dict(window=nan_window), dict(average=0), dict(average=65),
               dict(detector="median")):
        with pytest.raises(pkg.Gr4pmError):
            pkg.Spectrogram(**kw)
    assert L.gr4pm_spectrum_float_run() == 64
    sg = pkg.Spectrogram(hop=2048, average=64, detector="max")  # the largest hop and average are fine
    assert sg.rows(64 * 2048 - 1) == 0 and sg.rows(64 * 2048) == 1
    # reset() returns to the fresh stream from inside a row and inside a segment
    x = gref.stimulus(40000)
    want = run(pkg, x, 1000, 3)
    sg = pkg.Spectrogram(hop=1000, average=3)
    sg.process_bulk(dev(x[:7777]))
    sg.reset()
    assert sg.rows_done == 0
    assert np.array_equal(bits(run(pkg, x, 1000, 3, sg=sg)), bits(want))


BANDS = [(100, 138), (2000, 138), (0, 2048), (77, 1)]


def test_band_power(pkg):
    import torch
    n, hop = 40000, 1024
    sg = pkg.Spectrogram(hop=hop)
    rows = sg.process_bulk(dev(gref.stimulus(n)))
    assert tuple(rows.shape) == (38, N)
    got = sg.band_power(rows, BANDS)
    assert got.dtype == torch.float64 and tuple(got.shape) == (4, 38)
    want = gref.band_power(host(rows), BANDS)  # numpy's double sum of the same float32 rows
    g = host(got)
    for b, (_, n_bins) in enumerate(BANDS):
        rel = np.abs(g[b] - want[b]) / want[b]
        print(f"band {BANDS[b]}: worst relative error {rel.max():.3e}, bound {n_bins * 2.0 ** -53:.3e}")
        assert np.all(rel <= n_bins * 2.0 ** -53)
    assert np.array_equal(g[3], host(rows)[:, 77].astype(np.float64))
    # two identical calls give identical bits; find_carriers' structured array is taken as it is
    assert np.array_equal(host(sg.band_power(rows, BANDS)).view(np.uint64), g.view(np.uint64))
    carriers = np.zeros(2, dtype=[("frequency", "<f8"), ("first_bin", "<u8"), ("n_bins", "<u8")])
    carriers["first_bin"], carriers["n_bins"] = [100, 2000], [138, 138]
    assert np.array_equal(host(sg.band_power(rows, carriers)).view(np.uint64), g[:2].view(np.uint64))
    # more rows than one workgroup's four, a count that is no multiple of four, and no row at all
    many = torch.cat([rows] * 3, dim=0)[:110].contiguous()
    assert np.array_equal(host(sg.band_power(many, BANDS))[:, 76:110].view(np.uint64), g[:, :34].view(np.uint64))
    assert tuple(sg.band_power(rows[:0], BANDS).shape) == (4, 0)
    assert tuple(sg.band_power(rows, []).shape) == (0, 38)
    for bad in ([(100, 0)], [(100, 2049)], [(2048, 1)], [(0, 1)] * 65):
        with pytest.raises(pkg.Gr4pmError):
            sg.band_power(rows, bad)
    assert tuple(sg.band_power(rows, [(2047, 2048)] * 64).shape) == (64, 38)  # 64 bands are fine
