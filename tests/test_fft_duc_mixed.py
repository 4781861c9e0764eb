"""The MixedFftDuc block on the GPU against the float64 statement of its definition (tests/_fft_duc_mixed_ref.py) within the
derived first-order bound (device_bound there), and its exact properties: the FftDuc's bits for equal
interpolations and for one row, the same bits under any cutting into calls of whole slots, reset, rows in isolation, a row
of gain 0, zeros in giving zeros out, short calls, flush, pack and refusals.

Shapes: 5 hop / Imax + 1 slots at tests/test_fft_duc_mixed_ref.py's DEVICE_CASES, with section 27's stimulus, taps,
frequencies (both sides of a 64-bin boundary, on a bin, half-way between bins, slices across +-0.5) and gains, start_index
2^40 + 3.  The columns of the input behind a row's items hold NaN: they must not be read.

Measured on MI355X, worst error over bound per case, in DEVICE_CASES' order: 0.0019, 0.0018, 0.0026, 0.0006."""
import ctypes as C
import functools

import numpy as np
import pytest

import _fft_duc_mixed_ref as mref
import test_fft_duc_mixed_ref as cpu
import test_fft_duc_ref as uni
from _frontend import bits, dev, host, load_package

pytestmark = pytest.mark.gpu

N = mref.N
START = cpu.START
CASES = cpu.DEVICE_CASES
ISOLATION = ((64, 4, 64, 16), 1024, (2, 2, 2, 2))


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@functools.lru_cache(maxsize=None)
def setting(Is, V, Rs):
    """(rows complex64, taps float32, frequencies, gains), computed once per case and left unchanged"""
    rows = [r.astype(np.complex64) for r in cpu.rows_for(Is, V)]
    hs = [h.astype(np.float32) for h in cpu.taps_for(Is, V)]
    for a in rows + hs:
        a.setflags(write=False)
    return rows, hs, uni.device_freqs(len(Is)), uni.device_gains(len(Is))


@functools.lru_cache(maxsize=None)
def reference(Is, V, Rs):
    rows, hs, f, g = setting(Is, V, Rs)
    want = mref.mixed_fft_duc64(rows, hs, Is, f, g, V=V, Rs=Rs, start=START)
    bound = mref.device_bound(rows, hs, Is, f, g, V, Rs, start=START)
    want.setflags(write=False), bound.setflags(write=False)
    return want, bound


def make(pkg, Is, V, Rs, gains=None):
    _, hs, f, g = setting(Is, V, Rs)
    return pkg.MixedFftDuc(f, Is, gains=g if gains is None else gains, taps=hs, overlap=V, images=Rs, start_index=START)


def window(rows, Is, at, step):
    """[K, n_cols] complex64: row k's items of the slots [at, at + step) at the front of the row, NaN behind them"""
    Imax = max(Is)
    n = [step * Imax // I for I in Is]
    a = np.full((len(Is), max(n + [0])), np.nan + 1j * np.nan, dtype=np.complex64)
    for k, I in enumerate(Is):
        a[k, :n[k]] = rows[k][at * Imax // I:at * Imax // I + n[k]]
    return a


def run(block, rows, Is, cuts=()):
    """the rows through the block in calls of `cuts` slots, then the rest; the samples joined, on the host"""
    import torch
    slots, at, parts = mref.slots_of(rows, Is), 0, []
    before = block.pending
    for c in list(cuts) + [slots]:
        if at >= slots and parts:
            break
        step = min(c, slots - at)
        want = block.output_items(step)
        assert list(block.items_for(step)) == mref.items_for(Is, step)
        x = block.process_bulk(dev(window(rows, Is, at, step)), slots=step)
        assert x.shape[0] == want
        parts.append(x)
        at += step
        assert block.pending == (before + at) % (block.hop // block.slot)
    return host(torch.cat(parts))


@functools.lru_cache(maxsize=None)
def one_call(Is, V, Rs):
    out = run(make(load_package(), Is, V, Rs), setting(Is, V, Rs)[0], Is)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("Is,V,Rs", CASES)
def test_against_float64(pkg, Is, V, Rs):
    f = setting(Is, V, Rs)[2]
    want, bound = reference(Is, V, Rs)
    b = make(pkg, Is, V, Rs)
    assert (b.hop, b.overlap, b.pending, b.slot) == (N - V, V, 0, max(Is))
    assert list(b.interpolations) == list(Is) and list(b.images) == list(Rs)
    assert np.array_equal(b.frequencies, [mref.frequency_word(x) / 2.0 ** 32 - (mref.frequency_word(x) >= 1 << 31) for x in f])
    got = one_call(Is, V, Rs)
    assert got.shape == want.shape == (5 * (N - V),)
    err = np.abs(got.astype(np.complex128) - want)
    print(f"I {Is[:6]} V {V} R {Rs[:6]} K {len(Is)}: worst error / bound {np.max(err / bound):.4f}, worst error {np.max(err):.3e} "
          f"of {np.max(np.abs(want)):.3f}")
    assert np.all(np.isfinite(got.view(np.float32)))
    assert np.all(err <= bound)


def test_equal_interpolations_are_the_fft_duc_bit_for_bit(pkg):
    I, V, R, K = 16, 256, 2, 9
    Is, Rs = (I,) * K, (R,) * K
    rows, hs, f, g = setting(Is, V, Rs)
    got = one_call(Is, V, Rs)
    u = pkg.FftDuc(f, I, gains=g, taps=hs[0], overlap=V, images=R, start_index=START)
    want = host(u.process_bulk(dev(np.stack(rows))))
    assert want.shape == (5 * (N - V),) and np.any(want) and np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("I", cpu.CYCLE)
def test_one_row_is_the_fft_duc_bit_for_bit(pkg, I):
    Is, V, Rs = (I,), 1024, (2,)
    rows, hs, f, g = setting(Is, V, Rs)
    u = pkg.FftDuc(f, I, gains=g, taps=hs[0], overlap=V, images=2, start_index=START)
    want = host(u.process_bulk(dev(rows[0])))
    assert want.shape == (5 * (N - V),) and np.array_equal(bits(one_call(Is, V, Rs)), bits(want))


@pytest.mark.parametrize("Is,V,Rs", CASES)
def test_call_cuts_give_the_same_bits(pkg, Is, V, Rs):
    hs_, Bs = (N - V) // max(Is), N // max(Is)
    got = run(make(pkg, Is, V, Rs), setting(Is, V, Rs)[0], Is, cuts=(1, hs_ - 1, hs_, Bs + 1))
    assert np.array_equal(bits(got), bits(one_call(Is, V, Rs)))


def test_reset_reproduces_the_first_run(pkg):
    Is, V, Rs = CASES[0]
    rows = setting(Is, V, Rs)[0]
    b = make(pkg, Is, V, Rs)
    first = run(b, rows, Is, cuts=(7,))
    b.reset()
    assert b.pending == 0
    again = run(b, rows, Is, cuts=((N - V) // max(Is) + 3, 2))
    assert np.array_equal(bits(first), bits(again)) and np.array_equal(bits(first), bits(one_call(Is, V, Rs)))


def test_the_slowest_rows_alone_are_the_fft_duc(pkg):
    """the other rows fed zeros add +-0 products in ascending k, which leave every non-zero value as it is"""
    Is, V, Rs = ISOLATION
    rows, hs, f, g = setting(Is, V, Rs)
    alone = [r if I == 64 else np.zeros_like(r) for r, I in zip(rows, Is)]
    got = run(make(pkg, Is, V, Rs), alone, Is)
    u = pkg.FftDuc([f[0], f[2]], 64, gains=[g[0], g[2]], taps=hs[0], overlap=V, images=2, start_index=START)
    want = host(u.process_bulk(dev(np.stack([rows[0], rows[2]]))))
    assert np.any(want) and np.array_equal(got, want)


def test_a_row_of_gain_zero_changes_no_value(pkg):
    Is, V, Rs = ISOLATION
    rows, hs, f, g = setting(Is, V, Rs)
    g0 = list(g)
    g0[1] = 0.0
    with_zero = run(make(pkg, Is, V, Rs, gains=g0), rows, Is)
    keep = [0, 2, 3]
    without = run(pkg.MixedFftDuc([f[k] for k in keep], [Is[k] for k in keep], gains=[g[k] for k in keep], taps=[hs[k] for k in keep],
                                  overlap=V, images=2, start_index=START), [rows[k] for k in keep], [Is[k] for k in keep])
    assert np.any(with_zero) and np.array_equal(with_zero, without)
    assert not np.array_equal(with_zero, one_call(Is, V, Rs))


@pytest.mark.parametrize("Is,V,Rs", [CASES[0], CASES[2]])
def test_rows_of_zeros_give_exact_zeros(pkg, Is, V, Rs):
    Imax, hop = max(Is), N - V
    hs_, Bs = hop // Imax, N // Imax
    lo, hi = hs_ + 1, hs_ + 1 + Bs + hs_  # in slots: at least one segment's N samples lie in [lo, hi) slots
    rows = [np.array(r) for r in setting(Is, V, Rs)[0]]
    for r, I in zip(rows, Is):
        r[lo * Imax // I:hi * Imax // I] = 0
    got = run(make(pkg, Is, V, Rs), rows, Is)
    zero_segments = [s for s in range(5) if s * hop - V >= lo * Imax and s * hop - V + N <= hi * Imax]
    assert len(zero_segments) >= 1
    for s in zero_segments:
        assert not np.any(got[s * hop:(s + 1) * hop].view(np.float32)), s
    assert np.any(got[:hop]) and np.any(got[-hop:])


def test_a_call_shorter_than_a_hop_yields_nothing_and_the_next_completes(pkg):
    Is, V, Rs = CASES[1]
    rows = setting(Is, V, Rs)[0]
    Imax, hs_ = max(Is), (N - V) // max(Is)
    b = make(pkg, Is, V, Rs)
    assert b.output_items(hs_ // 2) == 0
    x = b.process_bulk(dev(window(rows, Is, 0, hs_ // 2)), slots=hs_ // 2)
    assert tuple(x.shape) == (0,) and b.pending == hs_ // 2
    assert b.output_items(hs_) == N - V
    rest = run(b, [r[(hs_ // 2) * Imax // I:] for r, I in zip(rows, Is)], Is, cuts=(hs_,))
    assert np.array_equal(bits(rest), bits(one_call(Is, V, Rs)))


@pytest.mark.parametrize("Is,V,Rs", [CASES[1], CASES[2]])
def test_flush_is_the_zeros_fed_by_hand(pkg, Is, V, Rs):
    import torch
    rows, hs = setting(Is, V, Rs)[:2]
    Imax, hop = max(Is), N - V
    hs_ = hop // Imax
    slots = mref.slots_of(rows, Is)
    a, b = make(pkg, Is, V, Rs), make(pkg, Is, V, Rs)
    assert a.flush_items() == 0 and tuple(a.flush().shape) == (0,)
    run(a, rows, Is), run(b, rows, Is)
    # row k's last item reaches the sample (n_k - 1) I_k + L_k - 1: so many samples must be out, in whole segments
    need = max((r.size - 1) * I + h.size for r, I, h in zip(rows, Is, hs))
    segments = -(-need // hop)
    zeros = segments * hs_ - slots
    assert a.flush_items() == zeros and zeros > 0
    tail = host(a.flush())
    cols = zeros * Imax // min(Is)
    by_hand = host(b.process_bulk(torch.zeros((len(Is), cols), dtype=torch.complex64, device="cuda"), slots=zeros))
    assert tail.shape == (segments * hop - 5 * hop,) and np.array_equal(bits(tail), bits(by_hand))
    assert a.pending == b.pending == 0
    # the stream goes on behind it
    more = [r[:(hs_ + 1) * Imax // I] for r, I in zip(rows, Is)]
    assert np.array_equal(bits(run(a, more, Is)), bits(run(b, more, Is)))


def test_pack_of_ragged_rows_is_the_hand_padded_array(pkg):
    Is, V, Rs = CASES[0]
    rows = setting(Is, V, Rs)[0]
    Imax = max(Is)
    lengths = [5, 2 * (Imax // Is[1]) + 1, 3, 40]  # one slot for row 0 (I = 4), three for rows 1 and 2, five for row 3 (I = 8)
    ragged = [r[:n] for r, n in zip(rows, lengths)]
    b = make(pkg, Is, V, Rs)
    v, slots = b.pack([dev(r) for r in ragged])
    want_slots = max(-(-n // (Imax // I)) for n, I in zip(lengths, Is))
    by_hand = np.zeros((len(Is), want_slots * Imax // min(Is)), dtype=np.complex64)
    for k, r in enumerate(ragged):
        by_hand[k, :r.size] = r
    assert slots == want_slots == 5 and np.array_equal(bits(host(v)), bits(by_hand))
    # and it goes through: with zero slots up to a hop behind it, the samples of the hand-padded rows
    fill = (N - V) // Imax
    zeros = dev(np.zeros((len(Is), fill * Imax // min(Is)), dtype=np.complex64))
    got = np.concatenate([host(b.process_bulk(v, slots)), host(b.process_bulk(zeros, fill))])
    padded = [np.concatenate([by_hand[k, :slots * Imax // I], np.zeros(fill * Imax // I, np.complex64)]) for k, I in enumerate(Is)]
    want = run(make(pkg, Is, V, Rs), padded, Is)
    assert want.size == N - V and np.any(want) and np.array_equal(bits(got), bits(want))


def test_refusals_leave_the_handle_usable(pkg):
    import torch
    from gr4_packet_modem_amd import _abi
    L = pkg.lib()
    Is, V, Rs = CASES[0]
    rows, hs, f, g = setting(Is, V, Rs)
    K = len(Is)
    nan_taps = [np.array(h) for h in hs]
    nan_taps[2][7] = np.nan
    ok = dict(frequencies=f, interpolations=Is, gains=g, taps=hs, overlap=V, images=Rs)
    for bad in (dict(interpolations=(4, 16, 64, 5)), dict(interpolations=(2, 16, 64, 8)), dict(interpolations=(4, 16, 128, 8)),
                dict(interpolations=(4, 16, 64)), dict(images=(2, 2, 3, 2)), dict(images=0), dict(images=(8, 2, 2, 2)),
                dict(images=(2, 2)), dict(overlap=V + 32), dict(overlap=N - 64 + 64), dict(overlap=0),
                dict(frequencies=[], interpolations=[], gains=None, taps=None, images=2),
                dict(frequencies=[0.01] * 65, interpolations=[16] * 65, gains=None, taps=None, images=2),
                dict(frequencies=[0.1, np.nan, 0.2, 0.3]), dict(gains=[1.0] * (K - 1)), dict(gains=[np.nan] * K), dict(taps=nan_taps),
                dict(taps=hs[:3]), dict(taps=None, taps_per_phase=0), dict(taps=None, taps_per_phase=40)):
        with pytest.raises(pkg.Gr4pmError):
            pkg.MixedFftDuc(**{**ok, **bad})
    # the overlap is too low for one row only: 1000 taps on the I = 4 row beside an I = 64 row
    long_taps = np.resize(hs[0], 1000)
    with pytest.raises(pkg.Gr4pmError, match="row 0"):
        pkg.MixedFftDuc([0.1, 0.2], (4, 64), taps=[long_taps, hs[2]], overlap=768)
    assert pkg.MixedFftDuc([0.1, 0.2], (4, 64), taps=[long_taps, hs[2]]).overlap == 1024
    # NULL arrays at create
    fa = np.asarray(f, dtype=np.float64)
    ia = np.asarray(Is, dtype=np.uintp)
    for freqs, interps in ((None, ia.ctypes.data_as(C.c_void_p)), (fa.ctypes.data_as(C.c_void_p), None)):
        hd = C.c_void_p(0x1234)
        p = _abi.FftDucMixedParams(K, interps, freqs, None, None, None, 12, None, -1, 0, None)
        assert L.gr4pm_fft_duc_mixed_create(C.byref(p), C.byref(hd)) == -1
        assert hd.value is None

    b = make(pkg, Is, V, Rs)
    slots = mref.slots_of(rows, Is)
    d = dev(window(rows, Is, 0, slots))
    cols = d.shape[1]
    samples = b.output_items(slots)
    out = torch.empty(samples, dtype=torch.complex64, device="cuda")
    n = C.c_size_t(77)
    call = lambda inp, stride, u, o, cap: L.gr4pm_fft_duc_mixed_process(b._h, inp, stride, u, o, cap, C.byref(n))
    assert call(None, cols, slots, out.data_ptr(), samples) == -1 and n.value == 0            # no input
    assert call(d.data_ptr(), cols, slots, None, samples) == -1 and n.value == 0              # no output
    assert call(d.data_ptr(), cols - 1, slots, out.data_ptr(), samples) == -1 and n.value == 0   # a stride below the longest row
    assert call(d.data_ptr(), cols, slots, out.data_ptr(), samples - 1) == -5 and n.value == 0   # no room
    many = (1 << 40) // (max(Is) // min(Is)) + 1
    assert call(d.data_ptr(), 1 << 41, many, out.data_ptr(), samples) == -5 and n.value == 0     # 2^40 items in the longest row
    with pytest.raises(pkg.Gr4pmError):
        b.output_items(many)
    with pytest.raises(pkg.Gr4pmError):
        b.items_for(many)
    with pytest.raises(pkg.Gr4pmError):
        b.process_bulk(d, out=out[:samples - 1])
    with pytest.raises(pkg.Gr4pmError):
        b.process_bulk(d[:K - 1])
    with pytest.raises(pkg.Gr4pmError):
        b.process_bulk(d, slots=slots + 1)
    assert b.output_items(slots) == samples and b.pending == 0  # nothing was taken
    assert np.array_equal(bits(run(b, rows, Is)), bits(one_call(Is, V, Rs)))
