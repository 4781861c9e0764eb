"""The RowResampler on the GPU (gr4pm_row_resampler): within the derived first-order bound of the
float64 restatement over every (Q, P), step, row length, phase0 and frequency word of the list; the exact properties (the
identity prototype, continuation at the tile's edges, a row alone, 70 rows as 64 + 6, the same bits twice, nothing read
behind a length, +0 behind M_r, NULL lengths, wide strides); the Ddc's bits for an integer step; and every refusal.

Rows are seeded random complex64 of at most 5000 items."""
import ctypes as C

import numpy as np
import pytest

import _row_resampler_ref as ref
from _frontend import bits, dev, host, load_package

pytestmark = pytest.mark.gpu

TWO32 = 1 << 32
N = 5000
SIZES = [(32, 12), (2, 1), (256, 16), (64, 3)]
STEPS = [TWO32, round(0.8929 * TWO32), round(2.2727 * TWO32), TWO32 // 64, 64 * TWO32, TWO32 + 1]
PHASES = [0, TWO32 // 2, 3 * TWO32 + TWO32 // 4]
WORDS = [0, round(0.003 * TWO32), -round(0.003 * TWO32), -(1 << 31)]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def row_lengths(P):
    return [0, 1, P - 1, P, 255, 257, N]


def rows_of(n_rows, n=N, seed=21):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n_rows, n)) + 1j * rng.standard_normal((n_rows, n))).astype(np.complex64)


def taps_of(Q, P):
    """the design with something random mixed in: every tap matters"""
    rng = np.random.default_rng(Q + P)
    return (ref.kaiser_taps64(Q, P) + 0.05 * rng.standard_normal(Q * P)).astype(np.float32)


def assert_padding(rows, lens):
    for r, M in enumerate(lens):
        assert not bits(rows[r, M:]).any(), f"row {r}: an item at or beyond M_r = {M} is not +0"


# ---- against the float64 restatement ----

WORST = {}


N_COLS = 6144


def bound_rows(P):
    """the 21 rows of the comparison: every length of row_lengths(P) at every phase0 of PHASES"""
    lengths = row_lengths(P) * len(PHASES)
    return lengths, [PHASES[r // 7] for r in range(len(lengths))], rows_of(len(lengths))


def bound_call(rs, xd, lengths, phase0, k):
    """call k of the comparison, at STEPS[k] with the frequency words rotated by k: the [21, N_COLS] array on the host,
    the lengths the call reported and the words"""
    freqs = [WORDS[(r + k) % len(WORDS)] for r in range(len(lengths))]
    y, lens = rs.process_rows(xd, lengths, [STEPS[k]] * len(lengths), phase0, freqs, n_cols=N_COLS)
    return host(y), lens, freqs


def bound_output(Q, P, k):
    """bound_call's array from a handle of its own"""
    lengths, phase0, x = bound_rows(P)
    return bound_call(load_package().RowResampler(phases=Q, taps=taps_of(Q, P)), dev(x), lengths, phase0, k)[0]


@pytest.mark.parametrize("Q,P", SIZES)
def test_within_the_derived_bound_of_float64(pkg, Q, P):
    h = taps_of(Q, P)
    rs = pkg.RowResampler(phases=Q, taps=h)
    lengths, phase0, x = bound_rows(P)
    xd = dev(x)
    worst = 0.0
    for k, step in enumerate(STEPS):
        n_cols = N_COLS
        y, lens, freqs = bound_call(rs, xd, lengths, phase0, k)
        assert y.shape == (len(lengths), n_cols)
        assert lens.tolist() == rs.output_lengths(lengths, [step] * len(lengths), phase0, n_cols=n_cols).tolist()
        assert_padding(y, lens)
        for r, n in enumerate(lengths):
            want = ref.resample64(x[r], n, h, Q, step, phase0[r], freqs[r], n_cols=n_cols)
            assert lens[r] == want.size == ref.output_items(n, P, step, phase0[r], n_cols)
            bound = ref.error_bound(x[r], n, h, Q, step, phase0[r], n_cols=n_cols)
            err = np.abs(y[r, :want.size].astype(np.complex128) - want)
            assert np.all(np.isfinite(y[r]))
            live = bound > 0
            assert np.all(y[r, :want.size][~live] == 0), "an item whose window is all zeros is not zero"
            if live.any():
                worst = max(worst, float(np.max(err[live] / bound[live])))
            assert np.all(err <= bound), (Q, P, step, r, n, float(np.max(err[live] / bound[live])))
    WORST[(Q, P)] = worst
    print(f"RowResampler ({Q}, {P}): worst error / bound = {worst:.3f}")


# ---- exact properties ----

def test_identity_prototype_returns_the_row(pkg):
    Q, P = 32, 4
    h = np.zeros(Q * P, np.float32)
    h[0] = 1.0
    x = rows_of(3, 1500, seed=5)
    assert np.all(x.real != 0) and np.all(x.imag != 0)
    lengths = [1500, 1, 700]
    y, lens = pkg.RowResampler(phases=Q, taps=h).process_rows(dev(x), lengths, [TWO32] * 3)
    y = host(y)
    assert lens.tolist() == [n + P - 1 for n in lengths] and y.shape[1] == 2048
    for r, n in enumerate(lengths):
        assert np.array_equal(bits(y[r, :n]), bits(x[r, :n]))
        assert np.all(y[r, n:] == 0)


@pytest.mark.parametrize("step", [round(0.8929 * TWO32), round(2.2727 * TWO32), 64 * TWO32])
def test_continuation_is_bit_exact_at_the_tile_edges(pkg, step):
    Q, P = 32, 12
    rs = pkg.RowResampler(phases=Q, taps=taps_of(Q, P))
    n = N if step < 8 * TWO32 else 3 * N
    x = dev(rows_of(1, n, seed=8))
    T = rs.tile_items([step])
    phase0, freq = TWO32 // 3, round(0.003 * TWO32)
    full, lens = rs.process_rows(x, [n], [step], [phase0], [freq])
    full, M = host(full)[0], int(lens[0])
    assert M > T + 1 + 16, (M, T)
    for m0 in (1, T - 1, T, T + 1):
        part, pl = rs.process_rows(x, [n], [step], [phase0 + m0 * step], [freq])
        assert int(pl[0]) == M - m0
        assert np.array_equal(bits(host(part)[0, :M - m0]), bits(full[m0:M])), (step, T, m0)


def seventy_rows(pkg):
    """70 rows of 600 items, every one with a length, a step, a phase0 and a word of its own, and the call on all of them
    (64 + 6 through the ABI)"""
    Q, P = 32, 12
    rs = pkg.RowResampler(phases=Q, taps=taps_of(Q, P))
    R = 70
    xd = dev(rows_of(R, 600, seed=9))
    rng = np.random.default_rng(10)
    lengths = [int(v) for v in rng.integers(0, 601, R)]
    steps = [int(v) for v in rng.integers(TWO32 // 2, 3 * TWO32, R)]
    phase0 = [int(v) for v in rng.integers(0, 4 * TWO32, R)]
    freqs = [int(v) for v in rng.integers(-(1 << 31), 1 << 31, R)]
    all_rows, all_lens = rs.process_rows(xd, lengths, steps, phase0, freqs, n_cols=2048)
    return rs, xd, lengths, steps, phase0, freqs, all_rows, all_lens


def seventy_rows_output():
    return host(seventy_rows(load_package())[6])


def test_rows_alone_split_calls_and_repeats(pkg):
    rs, xd, lengths, steps, phase0, freqs, all_rows, all_lens = seventy_rows(pkg)
    again, again_lens = rs.process_rows(xd, lengths, steps, phase0, freqs, n_cols=2048)
    all_rows, again = host(all_rows), host(again)
    assert np.array_equal(bits(all_rows), bits(again)) and all_lens.tolist() == again_lens.tolist()
    assert_padding(all_rows, all_lens)
    for lo, hi in ((0, 64), (64, 70), (0, 6)):
        part, pl = rs.process_rows(xd[lo:hi], lengths[lo:hi], steps[lo:hi], phase0[lo:hi], freqs[lo:hi], n_cols=2048)
        assert np.array_equal(bits(host(part)), bits(all_rows[lo:hi])) and pl.tolist() == all_lens[lo:hi].tolist()
    for r in range(6):
        one, ol = rs.process_rows(xd[r:r + 1], lengths[r:r + 1], steps[r:r + 1], phase0[r:r + 1], freqs[r:r + 1], n_cols=2048)
        assert np.array_equal(bits(host(one)[0]), bits(all_rows[r])), r
        assert int(ol[0]) == int(all_lens[r])


def test_nothing_is_read_behind_a_length_and_the_output_may_hold_anything(pkg):
    import torch
    Q, P = 32, 12
    rs = pkg.RowResampler(phases=Q, taps=taps_of(Q, P))
    lengths = [1, 255, 300, 0]
    x = rows_of(4, 300, seed=12)
    padded = x.copy()
    for r, n in enumerate(lengths):
        padded[r, n:] = 0
    dirty = x.copy()
    for r, n in enumerate(lengths):
        dirty[r, n:] = np.nan + 1j * np.nan
    steps = [round(0.8929 * TWO32), round(2.2727 * TWO32), TWO32, TWO32]
    freqs = [5, -7, 0, 3]
    want, wl = rs.process_rows(dev(padded), None, steps, None, freqs, n_cols=2048)  # no lengths: the full rows
    want = host(want)
    out = torch.full((4, 2048), float("nan"), dtype=torch.complex64, device="cuda")
    got, gl = rs.process_rows(dev(dirty), lengths, steps, None, freqs, n_cols=2048, out=out)
    got = host(got)
    assert np.all(np.isfinite(got))
    assert_padding(got, gl)
    assert gl.tolist() == rs.output_lengths(lengths, steps).tolist()
    for r in range(4):
        M = int(gl[r])
        assert M <= int(wl[r])
        assert np.array_equal(got[r, :M], want[r, :M]), r  # the zero-padded row's values (a zero's sign aside)


def test_strides_above_the_column_counts(pkg):
    import torch
    Q, P = 64, 3
    rs = pkg.RowResampler(phases=Q, taps=taps_of(Q, P))
    x = rows_of(5, 400, seed=13)
    wide = torch.full((5, 1000), float("nan"), dtype=torch.complex64, device="cuda")
    wide[:, :400] = dev(x)
    steps, lengths = [round(1.37 * TWO32)] * 5, [400, 399, 1, 0, 250]
    want, wl = rs.process_rows(dev(x), lengths, steps, n_cols=512)
    out = torch.full((5, 3000), float("nan"), dtype=torch.complex64, device="cuda")
    got, gl = rs.process_rows(wide[:, :400], lengths, steps, n_cols=512, out=out)
    assert got.shape == (5, 512) and got.stride(0) == 3000
    assert np.array_equal(bits(host(got)), bits(host(want))) and gl.tolist() == wl.tolist()
    assert torch.isnan(out[:, 512:].real).all(), "the call wrote beyond its columns"


# ---- the tie to the Ddc ----

@pytest.mark.parametrize("D", [1, 5])
def test_integer_steps_have_the_ddc_s_values(pkg, D):
    """step = D, phase0 = D - 1, freq = 0: mu = 0, so c_s = h[s Q] and item n is Ddc([0.0], D, taps=h[::Q])'s frame n: one
    accumulator, the taps ascending and the same rotator product on both sides.  The Ddc's complex multiply-accumulate
    adds the products with its taps' zero imaginary parts, which can only change a zero's sign."""
    Q, P = 32, 12
    h = taps_of(Q, P)
    x = rows_of(1, N, seed=14)
    y, lens = pkg.RowResampler(phases=Q, taps=h).process_rows(dev(x), [N], [D * TWO32], [(D - 1) * TWO32])
    want = host(pkg.Ddc([0.0], D, taps=np.ascontiguousarray(h[::Q])).process_bulk(dev(x[0])))[0]
    assert want.size == N // D and int(lens[0]) >= want.size
    assert np.array_equal(host(y)[0, :want.size], want)


# ---- refusals ----

def test_refusals_through_the_abi(pkg):
    import torch
    L = pkg.lib()
    invalid, overflow = -1, -5  # GR4PM_ERR_INVALID, GR4PM_ERR_OVERFLOW
    from gr4_packet_modem_amd import _abi
    rs = pkg.RowResampler()
    h = rs._handle()
    x = dev(rows_of(2, 64, seed=15))
    out = torch.full((2, 128), float("nan"), dtype=torch.complex64, device="cuda")
    ol = np.zeros(64, np.uint64)

    def records(n, step=TWO32, phase0=0, freq=0):
        rec = np.zeros(n, dtype=_abi.ROW_RECORD_DTYPE)
        rec["step"], rec["phase0"], rec["freq"] = step, phase0, freq
        return rec

    def call(n_rows=2, xp=x.data_ptr(), stride=64, n_cols=64, lengths=None, rec=None, outp=out.data_ptr(), out_stride=128,
             n_cols_out=128, olp=ol.ctypes.data_as(C.c_void_p)):
        rec = records(max(n_rows, 1)) if rec is None else rec
        lp = None if lengths is None else np.asarray(lengths, np.uint64).ctypes.data_as(C.c_void_p)
        return L.gr4pm_row_resampler_process(h, xp, stride, n_cols, lp, rec.ctypes.data_as(C.c_void_p), n_rows, outp, out_stride,
                                             n_cols_out, olp)

    ok = call()
    assert ok == 0 and ol[:2].tolist() == [64 + 11, 64 + 11]  # NULL lengths: every row has n_cols items
    want, _ = rs.process_rows(x, [64, 64], [TWO32, TWO32], n_cols=128)
    assert np.array_equal(bits(host(out)), bits(host(want)))
    assert L.gr4pm_row_resampler_process(None, x.data_ptr(), 64, 64, None, None, 1, out.data_ptr(), 128, 128, None) == invalid
    out.fill_(float("nan"))
    cases = [
        (overflow, dict(n_cols_out=(1 << 31) + 1, out_stride=1 << 32)),
        (invalid, dict(n_rows=65, rec=records(65))),
        (invalid, dict(lengths=[64, 65])),
        (invalid, dict(stride=63)),
        (invalid, dict(out_stride=127)),
        (invalid, dict(rec=records(2, step=(1 << 26) - 1))),
        (invalid, dict(rec=records(2, step=(1 << 38) + 1))),
        (invalid, dict(outp=None)),
        (invalid, dict(olp=None)),
        (invalid, dict(xp=None)),
        (overflow, dict(rec=records(2, phase0=1 << 63))),
        (overflow, dict(n_cols=1 << 32, stride=1 << 32, lengths=[64, TWO32 - 11])),
    ]
    for want, kw in cases:
        assert call(**kw) == want, kw
        assert pkg.lib().gr4pm_last_error()
    assert L.gr4pm_row_resampler_process(h, x.data_ptr(), 64, 64, None, None, 2, out.data_ptr(), 128, 128,
                                         ol.ctypes.data_as(C.c_void_p)) == invalid  # no records
    assert call(n_rows=0) == 0 and call(n_cols_out=0) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out.real).all(), "a refused or empty call enqueued something"
    assert call(xp=None, lengths=[0, 0]) == 0 and ol[:2].tolist() == [0, 0]  # no item: no input array is needed
    assert not bits(host(out)).any()

    hh = C.c_void_p()
    for q, p, taps in ((3, 4, None), (512, 1, None), (1, 4, None), (256, 17, None), (32, 0, np.ones(32, np.float32)),
                       (2, 1, np.array([1.0, np.nan], np.float32))):
        prm = _abi.RowResamplerParams(q, p, None if taps is None else taps.ctypes.data_as(C.c_void_p), None)
        assert L.gr4pm_row_resampler_create(C.byref(prm), C.byref(hh)) == invalid and not hh.value
    prm = _abi.RowResamplerParams(32, 0, None, None)  # NULL taps: the design with 12 taps per phase
    assert L.gr4pm_row_resampler_create(C.byref(prm), C.byref(hh)) == 0 and hh.value
    L.gr4pm_row_resampler_destroy(hh)


def test_refusals_through_the_class(pkg):
    import torch
    rs = pkg.RowResampler()
    x = dev(rows_of(2, 64, seed=16))
    good = dict(lengths=[64, 64], steps=[TWO32, TWO32])
    rs.process_rows(x, **good)
    for kw in (dict(good, lengths=[64, 65]), dict(good, steps=[TWO32, (1 << 26) - 1]), dict(good, steps=[(1 << 38) + 1, TWO32]),
               dict(good, steps=[TWO32]), dict(good, phase0=[0, 1 << 63]), dict(good, freqs=[0, 1 << 31]),
               dict(good, n_cols=(1 << 31) + 1, out=torch.empty((2, 0), dtype=torch.complex64, device="cuda")),
               dict(good, out=torch.empty((2, 100), dtype=torch.complex64, device="cuda"), n_cols=128)):
        with pytest.raises(pkg.Gr4pmError):
            rs.process_rows(x, **kw)
    with pytest.raises(TypeError):
        rs.process_rows(x.to(torch.complex128), **good)
    with pytest.raises(TypeError):
        rs.process_rows(x.cpu(), **good)
    y, lens = rs.process_rows(x[:0], [], [])
    assert y.shape == (0, 0) and lens.size == 0
