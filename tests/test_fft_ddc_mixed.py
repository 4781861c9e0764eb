"""The MixedFftDdc block on the GPU against the float64 statement of its definition (tests/_fft_ddc_mixed_ref.py) within the
derived first-order bound (device_bound there: DESIGN.md section 25's, per channel), and its exact properties: with all
decimations equal the FftDdc's bits; the channels at Dmax inside a mixed handle the FftDdc's bits; the same bits under any
cutting of the stream into calls; integer ingest, reset, zeros in giving zeros out, short calls, +0 behind every row,
refusals.

Shapes: n = 5 hop + 77 samples at the (D_k, V, R_k) of tests/test_fft_ddc_mixed_ref.py's DEVICE_CASES, with its stimulus,
taps and frequencies.

Measured on MI355X, worst error over bound per case, in DEVICE_CASES' order: 0.0030, 0.0119, 0.0052, 0.0125."""
import ctypes as C
import functools

import numpy as np
import pytest

import _fft_ddc_mixed_ref as mref
import _fft_ddc_ref as fref
import test_fft_ddc_mixed_ref as cpu
import test_fft_ddc_ref as one
from _frontend import bits, dev, exact_iq_forms, host, load_package

pytestmark = pytest.mark.gpu

N = fref.N
START = cpu.START
CASES = list(range(len(cpu.DEVICE_CASES)))
AT_DMAX = ((64, 4, 64, 16), 1024, (2, 2, 2, 2))


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@functools.lru_cache(maxsize=None)
def setting(case):
    """(D_k, V, R_k, x complex64, taps float32, frequencies, the float64 reference, the bound), computed once per case"""
    Ds, V, Rs = cpu.DEVICE_CASES[case]
    hop = N - V
    x = cpu.stimulus(5 * hop + 77).astype(np.complex64)
    hs = [h.astype(np.float32) for h in cpu.taps_for(Ds, V)]
    f = cpu.freqs_for(len(Ds))
    want = mref.mixed64(x, hs, Ds, f, V=V, Rs=Rs, start=START)
    bound = mref.device_bound(x, hs, Ds, f, V, Rs)
    for a in [x] + hs + want + bound:
        a.setflags(write=False)
    return Ds, V, Rs, x, hs, f, want, bound


def make(pkg, case, start=START):
    Ds, V, Rs, _, hs, f, _, _ = setting(case)
    return pkg.MixedFftDdc(f, Ds, taps=hs, overlap=V, images=Rs, start_index=start)


def run(block, x, cuts=(), scale=None):
    """x through the block in calls of the lengths `cuts`, then the rest; per row the frames of all calls joined, on the
    host.  Every call's lengths are what frames_for said, and behind them the rows hold +0."""
    d, lo, parts = dev(x), 0, [[] for _ in range(block.n_channels)]
    for c in list(cuts) + [len(x)]:
        if lo >= len(x) and lo > 0:
            break
        part = d[lo:lo + c]
        want = block.frames_for(part.shape[0])
        rows, lengths = block.process_bulk(part, scale=scale) if scale is not None else block.process_bulk(part)
        assert lengths.dtype == np.int64 and np.array_equal(lengths, want)
        assert tuple(rows.shape) == (block.n_channels, int(lengths.max()))
        r = host(rows)
        for k in range(block.n_channels):
            parts[k].append(r[k, :lengths[k]])
            assert not np.any(bits(r[k, lengths[k]:])), k  # +0, not -0
        lo += c
    return [np.concatenate(p) for p in parts]


@functools.lru_cache(maxsize=None)
def one_call(case):
    out = run(make(load_package(), case), setting(case)[3])
    for a in out:
        a.setflags(write=False)
    return out


def same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(bits(p), bits(q)) for p, q in zip(a, b))


@pytest.mark.parametrize("case", CASES, ids=cpu.CASE_IDS)
def test_against_float64(pkg, case):
    Ds, V, Rs, _, _, f, want, bound = setting(case)
    b = make(pkg, case)
    assert (b.hop, b.overlap) == (N - V, V) and list(b.decimations) == list(Ds)
    assert np.array_equal(b.frequencies, [fref.frequency_word(v) / 2.0 ** 32 - (fref.frequency_word(v) >= 1 << 31) for v in f])
    got = one_call(case)
    worst, worst_err = 0.0, 0.0
    for k, D in enumerate(Ds):
        assert got[k].shape == want[k].shape == (5 * (N - V) // D,)
        assert np.all(np.isfinite(got[k].view(np.float32)))
        err = np.abs(got[k].astype(np.complex128) - want[k])
        worst, worst_err = max(worst, float(np.max(err / bound[k]))), max(worst_err, float(np.max(err)))
    print(f"D {Ds[:5]}{'...' if len(Ds) > 5 else ''} V {V} R {Rs[:5]}: worst error / bound {worst:.4f}, worst error {worst_err:.3e}")
    for k in range(len(Ds)):
        assert np.all(np.abs(got[k].astype(np.complex128) - want[k]) <= bound[k]), k


def test_equal_decimations_are_the_fft_ddc_bit_for_bit(pkg):
    D, V, R, K = 16, 256, 2, 9
    hop = N - V
    x = cpu.stimulus(5 * hop + 77).astype(np.complex64)
    h = one.taps_for(D, V).astype(np.float32)
    f = one.device_freqs(K)
    got = run(pkg.MixedFftDdc(f, [D] * K, taps=[h] * K, overlap=V, images=R, start_index=START), x)
    want = host(pkg.FftDdc(f, D, taps=h, overlap=V, images=R, start_index=START).process_bulk(dev(x)))
    assert want.shape == (K, 5 * hop // D)
    assert same_bits(got, list(want))


def test_channels_at_dmax_are_the_fft_ddc_bit_for_bit(pkg):
    Ds, V, Rs = AT_DMAX
    hop = N - V
    x = cpu.stimulus(5 * hop + 77).astype(np.complex64)
    hs = [h.astype(np.float32) for h in cpu.taps_for(Ds, V)]
    got = run(pkg.MixedFftDdc(cpu.FREQS, Ds, taps=hs, overlap=V, images=Rs, start_index=START), x)
    at = [k for k, D in enumerate(Ds) if D == 64]
    assert np.array_equal(hs[at[0]], hs[at[1]])
    want = host(pkg.FftDdc([cpu.FREQS[k] for k in at], 64, taps=hs[at[0]], overlap=V, images=2, start_index=START).process_bulk(dev(x)))
    assert want.shape == (2, 5 * hop // 64)
    assert same_bits([got[k] for k in at], list(want))
    assert [g.size for g in got] == [5 * hop // D for D in Ds]


@pytest.mark.parametrize("case", CASES, ids=cpu.CASE_IDS)
def test_call_cuts_give_the_same_bits(pkg, case):
    V, x = setting(case)[1], setting(case)[3]
    hop = N - V
    cuts = [1, hop - 1, hop, N + 1]
    assert sum(cuts) < x.size
    assert same_bits(run(make(pkg, case), x, cuts), one_call(case))


@pytest.mark.parametrize("case", [0, 1], ids=cpu.CASE_IDS[:2])
def test_integer_iq_is_unpack_then_process(pkg, case):
    V = setting(case)[1]
    hop = N - V
    _, forms = exact_iq_forms(3 * hop + 77, 9)
    a, scale = forms[1]  # sc16
    unpacked = host(pkg.iq_unpack(dev(a), scale))
    want = run(make(pkg, case), unpacked)
    got = run(make(pkg, case), a, cuts=(hop // 3, hop + 5), scale=scale)
    assert [w.size for w in want] == [3 * hop // D for D in setting(case)[0]]
    assert same_bits(got, want)


def test_reset_reproduces_the_first_run(pkg):
    x = setting(0)[3]
    b = make(pkg, 0)
    first = run(b, x, cuts=(1000,))
    b.reset()
    again = run(b, x, cuts=(N - setting(0)[1] + 3, 17))
    assert same_bits(first, again) and same_bits(first, one_call(0))


def test_zeros_in_give_zeros_out(pkg):
    Ds, V = setting(0)[0], setting(0)[1]
    hop = N - V
    got = run(make(pkg, 0), np.zeros(3 * hop + 77, dtype=np.complex64))
    assert [g.size for g in got] == [3 * hop // D for D in Ds]
    assert not any(np.any(g.view(np.float32)) for g in got)


def test_a_call_shorter_than_a_segment_delivers_nothing_and_the_next_completes(pkg):
    Ds, V, x = setting(0)[0], setting(0)[1], setting(0)[3]
    hop = N - V
    b = make(pkg, 0)
    assert not np.any(b.frames_for(hop // 2))
    rows, lengths = b.process_bulk(dev(x[:hop // 2]))
    assert tuple(rows.shape) == (len(Ds), 0) and lengths.dtype == np.int64 and not np.any(lengths)
    assert list(b.frames_for(hop)) == [hop // D for D in Ds]
    assert same_bits(run(b, x[hop // 2:], cuts=(hop,)), one_call(0))


def test_out_filled_with_nan_comes_back_zero_padded(pkg):
    import torch
    Ds, V, x = setting(0)[0], setting(0)[1], setting(0)[3]
    longest = 5 * (N - V) // min(Ds)
    out = torch.full((len(Ds), longest + 3), float("nan"), dtype=torch.complex64, device="cuda")
    rows, lengths = make(pkg, 0).process_bulk(dev(x), out=out[:, 1:])  # rows that do not begin at the row stride
    assert rows.data_ptr() == out[:, 1:].data_ptr() and tuple(rows.shape) == (len(Ds), longest)
    assert list(lengths) == [5 * (N - V) // D for D in Ds]
    r, whole = host(rows), host(out)
    assert not np.any(np.isnan(r.view(np.float32)))
    for k in range(len(Ds)):
        assert np.array_equal(bits(r[k, :lengths[k]]), bits(one_call(0)[k]))
        assert not np.any(bits(r[k, lengths[k]:])), k
    # nothing outside the rows' [0, longest) was written
    assert np.all(np.isnan(whole[:, 0])) and np.all(np.isnan(whole[:, longest + 1:]))


def test_refusals_leave_the_handle_usable(pkg):
    import torch
    L = pkg.lib()
    Ds, V, Rs, x, hs, f, _, _ = setting(0)
    ok = dict(frequencies=f, decimations=Ds, taps=hs, overlap=V, images=Rs)
    long_taps = [np.ones(720, dtype=np.float32), np.ones(100, dtype=np.float32)]
    for bad in (dict(decimations=(4, 16, 64, 2)), dict(decimations=(3, 16, 64, 8)), dict(decimations=(3, 16, 64, 8), taps=None), dict(decimations=(4, 16, 128, 8)),
                dict(images=(2, 2, 2, 16)), dict(images=(8, 2, 2, 2)), dict(images=3), dict(overlap=V + 32), dict(overlap=N - 64 + 64),
                dict(frequencies=f[:3]), dict(frequencies=[0.1, np.nan, 0.2, 0.3]), dict(taps=hs[:3]),
                # L_0 - 1 = 719 <= 768, but beside D = 64 channel 0 needs 60 + 719 = 779 > 768
                dict(frequencies=f[:2], decimations=(4, 64), taps=long_taps, overlap=768, images=2)):
        with pytest.raises(pkg.Gr4pmError):
            pkg.MixedFftDdc(**{**ok, **bad})
    # the same taps at the overlap that takes them, and alone with their own decimation at 768
    assert pkg.MixedFftDdc(f[:2], (4, 64), taps=long_taps, images=2).overlap == 1024
    assert pkg.FftDdc(f[:1], 4, taps=long_taps[0], overlap=768).overlap == 768
    with pytest.raises(pkg.Gr4pmError, match="channel 0"):
        pkg.MixedFftDdc(f[:2], (4, 64), taps=long_taps, overlap=768)

    b = make(pkg, 0)
    K = len(Ds)
    d = dev(x)
    frames = int(b.frames_for(x.size).max())
    out = torch.empty((K, frames), dtype=torch.complex64, device="cuda")
    n = np.full(K, 77, dtype=np.uintp)
    np_ptr = n.ctypes.data_as(C.c_void_p)

    def call(inp, n_in, o, stride, cap):
        n[:] = 77
        return L.gr4pm_fft_ddc_mixed_process(b._h, inp, n_in, o, stride, cap, np_ptr)

    assert call(None, x.size, out.data_ptr(), frames, frames) == -1 and not np.any(n)          # no input
    assert call(d.data_ptr(), x.size, None, frames, frames) == -1 and not np.any(n)            # no output
    assert call(d.data_ptr(), x.size, out.data_ptr(), frames - 1, frames) == -1 and not np.any(n)  # a stride below the longest row
    assert call(d.data_ptr(), x.size, out.data_ptr(), frames, frames - 1) == -5 and not np.any(n)  # no room
    assert call(d.data_ptr(), (1 << 40) + 1, out.data_ptr(), frames, frames) == -5 and not np.any(n)  # 2^40 samples a call
    n[:] = 77
    assert L.gr4pm_fft_ddc_mixed_process_iq(b._h, d.data_ptr(), 9, 0.0, x.size, out.data_ptr(), frames, frames, np_ptr) == -1
    assert not np.any(n)
    with pytest.raises(pkg.Gr4pmError):
        b.frames_for((1 << 40) + 1)
    with pytest.raises(pkg.Gr4pmError):
        b.process_bulk(d, out=out[:, :frames - 1])
    assert int(b.frames_for(x.size).max()) == frames  # nothing was taken
    assert same_bits(run(b, x), one_call(0))
