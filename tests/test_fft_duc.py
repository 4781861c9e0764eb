"""The FftDuc block on the GPU against the float64 statement of its definition (tests/_fft_duc_ref.py) within the derived
first-order bound (device_bound there), and its exact properties: the same bits under any cutting
of the rows into calls, reset, zeros in giving zeros out, short calls, flush, refusals, and a row of gain 0.

Shapes: n = 5 hopI + 3 items per row at the (I, V, R, K) of tests/test_fft_duc_ref.py's DEVICE_CASES, with its stimulus,
taps, frequencies (both sides of a 64-bin boundary, on a bin, half-way between bins, slices across +-0.5) and gains.

Measured on MI355X, worst error over bound per case, in DEVICE_CASES' order: 0.0016, 0.0017, 0.0087, 0.0031, 0.0015."""
import ctypes as C
import functools

import numpy as np
import pytest

import _fft_duc_ref as fref
import test_fft_duc_ref as cpu
from _frontend import bits, dev, host, load_package

pytestmark = pytest.mark.gpu

N = fref.N
START = cpu.START
CASES = cpu.DEVICE_CASES


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@functools.lru_cache(maxsize=None)
def setting(I, V, R, K):
    """(v complex64 [K, n], taps float32, frequencies, gains, the float64 reference, the bound), computed once per case"""
    v = cpu.stimulus(K, cpu.items_for(I, V)).astype(np.complex64)
    h = cpu.taps_for(I, V).astype(np.float32)
    f, g = cpu.device_freqs(K), cpu.device_gains(K)
    want = fref.fft_duc64(v, h, I, f, g, V=V, R=R, start=START)
    bound = fref.device_bound(v, h, I, f, g, V, R, start=START)
    for a in (v, h, want, bound):
        a.setflags(write=False)
    return v, h, f, g, want, bound


def make(pkg, I, V, R, K, start=START, gains=None):
    _, h, f, g, _, _ = setting(I, V, R, K)
    return pkg.FftDuc(f, I, gains=g if gains is None else gains, taps=h, overlap=V, images=R, start_index=start)


def run(block, v, cuts=()):
    """the rows v through the block in calls of the lengths `cuts`, then the rest; the samples joined, on the host"""
    import torch
    d, lo, parts = dev(v), 0, []
    n = v.shape[1]
    before = block.pending
    for c in list(cuts) + [n]:
        if lo >= n and parts:
            break
        part = d[:, lo:lo + c]
        want = block.output_items(part.shape[1])
        x = block.process_bulk(part)
        assert x.shape[0] == want
        parts.append(x)
        lo += c
        assert block.pending == (before + min(lo, n)) % (block.hop // block.interpolation)
    return host(torch.cat(parts))


@functools.lru_cache(maxsize=None)
def one_call(I, V, R, K):
    out = run(make(load_package(), I, V, R, K), setting(I, V, R, K)[0])
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("I,V,R,K", CASES)
def test_against_float64(pkg, I, V, R, K):
    _, _, f, _, want, bound = setting(I, V, R, K)
    b = make(pkg, I, V, R, K)
    assert (b.hop, b.overlap, b.pending) == (N - V, V, 0)
    assert np.array_equal(b.frequencies, [fref.frequency_word(x) / 2.0 ** 32 - (fref.frequency_word(x) >= 1 << 31) for x in f])
    got = one_call(I, V, R, K)
    assert got.shape == want.shape == (5 * (N - V),)
    err = np.abs(got.astype(np.complex128) - want)
    print(f"I {I} V {V} R {R} K {K}: worst error / bound {np.max(err / bound):.4f}, worst error {np.max(err):.3e} "
          f"of {np.max(np.abs(want)):.3f}")
    assert np.all(np.isfinite(got.view(np.float32)))
    assert np.all(err <= bound)


@pytest.mark.parametrize("I,V,R,K", CASES)
def test_call_cuts_give_the_same_bits(pkg, I, V, R, K):
    v = setting(I, V, R, K)[0]
    hop_items, B = (N - V) // I, N // I
    got = run(make(pkg, I, V, R, K), v, cuts=(1, hop_items - 1, hop_items, B + 1))
    assert np.array_equal(bits(got), bits(one_call(I, V, R, K)))


def test_reset_reproduces_the_first_run(pkg):
    I, V, R, K = CASES[1]
    v = setting(I, V, R, K)[0]
    b = make(pkg, I, V, R, K)
    first = run(b, v, cuts=(100,))
    b.reset()
    assert b.pending == 0
    again = run(b, v, cuts=((N - V) // I + 3, 17))
    assert np.array_equal(bits(first), bits(again)) and np.array_equal(bits(first), bits(one_call(I, V, R, K)))


@pytest.mark.parametrize("I,V,R,K", [CASES[0], CASES[2]])
def test_rows_of_zeros_give_exact_zeros(pkg, I, V, R, K):
    hop_items, B = (N - V) // I, N // I
    v = np.array(setting(I, V, R, K)[0])
    lo, hi = hop_items + 3, hop_items + 3 + B + hop_items  # at least one segment's B items per row lie in [lo, hi)
    v[:, lo:hi] = 0
    got = run(make(pkg, I, V, R, K), v)
    zero_segments = [s for s in range(5) if s * hop_items - V // I >= lo and s * hop_items - V // I + B <= hi]
    assert len(zero_segments) >= 1
    hop = N - V
    for s in zero_segments:
        assert not np.any(got[s * hop:(s + 1) * hop].view(np.float32)), s
    assert np.any(got[:hop]) and np.any(got[-hop:])


def test_a_call_shorter_than_hop_items_yields_nothing_and_the_next_completes(pkg):
    I, V, R, K = CASES[1]
    v = setting(I, V, R, K)[0]
    hop_items = (N - V) // I
    b = make(pkg, I, V, R, K)
    assert b.output_items(hop_items // 2) == 0
    x = b.process_bulk(dev(v[:, :hop_items // 2]))
    assert tuple(x.shape) == (0,) and b.pending == hop_items // 2
    assert b.output_items(hop_items) == N - V
    rest = run(b, v[:, hop_items // 2:], cuts=(hop_items,))
    assert np.array_equal(bits(rest), bits(one_call(I, V, R, K)))


@pytest.mark.parametrize("I,V,R,K", [CASES[1], CASES[2]])
def test_flush_is_the_zeros_fed_by_hand(pkg, I, V, R, K):
    import torch
    v, h = setting(I, V, R, K)[:2]
    hop, hop_items = N - V, (N - V) // I
    n = v.shape[1]
    a, b = make(pkg, I, V, R, K), make(pkg, I, V, R, K)
    assert a.flush_items() == 0 and tuple(a.flush().shape) == (0,)
    run(a, v), run(b, v)
    # the last item reaches the sample (n - 1) I + L - 1: so many samples must be out, in whole segments
    segments = -(-((n - 1) * I + h.size) // hop)
    zeros = segments * hop_items - n
    assert a.flush_items() == zeros and zeros > 0
    tail = host(a.flush())
    by_hand = host(b.process_bulk(torch.zeros((K, zeros), dtype=torch.complex64, device="cuda")))
    assert tail.shape == (segments * hop - 5 * hop,) and np.array_equal(bits(tail), bits(by_hand))
    assert a.pending == b.pending == 0
    # the stream goes on behind it
    more = v[:, :hop_items + 1]
    assert np.array_equal(bits(run(a, more)), bits(run(b, more)))


def test_a_row_of_gain_zero_changes_no_bit(pkg):
    I, V, R, K = CASES[1]
    v, h, f, g = setting(I, V, R, K)[:4]
    keep = [k for k in range(K) if k != 4]  # row 4's slice overlaps its neighbours' (0.4999 beside -0.5)
    g0 = list(g)
    g0[4] = 0.0
    with_zero = run(pkg.FftDuc(f, I, gains=g0, taps=h, overlap=V, images=R, start_index=START), v)
    without = run(pkg.FftDuc([f[k] for k in keep], I, gains=[g[k] for k in keep], taps=h, overlap=V, images=R, start_index=START),
                  np.ascontiguousarray(v[keep]))
    assert np.any(with_zero) and np.array_equal(with_zero, without)


def test_refusals_leave_the_handle_usable(pkg):
    import torch
    from gr4_packet_modem_amd import _abi
    L = pkg.lib()
    I, V, R, K = CASES[1]
    v, h, f, g, _, _ = setting(I, V, R, K)
    nan_taps, inf_taps = np.array(h), np.array(h)
    nan_taps[7], inf_taps[0] = np.nan, np.inf
    ok = dict(frequencies=f, interpolation=I, gains=g, taps=h, overlap=V, images=R)
    for bad in (dict(interpolation=5), dict(interpolation=2), dict(interpolation=128), dict(images=3), dict(images=0),
                dict(images=2 * I), dict(overlap=V + 1), dict(overlap=(h.size - 2) // I * I), dict(overlap=N - 64 + I),
                dict(frequencies=[], gains=None), dict(frequencies=[0.01] * 65, gains=None), dict(frequencies=[0.1, np.nan], gains=None),
                dict(frequencies=[np.inf], gains=None), dict(gains=[1.0] * (K - 1)), dict(gains=[np.nan] * K), dict(taps=nan_taps),
                dict(taps=inf_taps)):
        with pytest.raises(pkg.Gr4pmError):
            pkg.FftDuc(**{**ok, **bad})
    with pytest.raises(pkg.Gr4pmError):
        pkg.fft_duc_taps(12)
    assert np.array_equal(pkg.fft_duc_taps(I), pkg.duc_taps(I))
    # NULL arrays at create
    fa = np.asarray(f, dtype=np.float64)
    for freqs in (None, fa.ctypes.data_as(C.c_void_p)):
        hd = C.c_void_p(0x1234)
        p = _abi.FftDucParams(K, I, freqs, None, h.ctypes.data_as(C.c_void_p), h.size if freqs is None else 0, 12, V, R, 0, None)
        assert L.gr4pm_fft_duc_create(C.byref(p), C.byref(hd)) == -1  # no frequencies; a prototype of 0 taps
        assert hd.value is None

    b = make(pkg, I, V, R, K)
    d = dev(v)
    n_in = v.shape[1]
    samples = b.output_items(n_in)
    out = torch.empty(samples, dtype=torch.complex64, device="cuda")
    n = C.c_size_t(77)
    call = lambda inp, stride, items, o, cap: L.gr4pm_fft_duc_process(b._h, inp, stride, items, o, cap, C.byref(n))
    assert call(None, n_in, n_in, out.data_ptr(), samples) == -1 and n.value == 0           # no input
    assert call(d.data_ptr(), n_in, n_in, None, samples) == -1 and n.value == 0             # no output
    assert call(d.data_ptr(), n_in - 1, n_in, out.data_ptr(), samples) == -1 and n.value == 0  # a stride below the items
    assert call(d.data_ptr(), n_in, n_in, out.data_ptr(), samples - 1) == -5 and n.value == 0  # no room
    assert call(d.data_ptr(), (1 << 40) + 1, (1 << 40) + 1, out.data_ptr(), samples) == -5 and n.value == 0  # 2^40 items a call
    with pytest.raises(pkg.Gr4pmError):
        b.output_items((1 << 40) + 1)
    with pytest.raises(pkg.Gr4pmError):
        b.process_bulk(d, out=out[:samples - 1])
    with pytest.raises(pkg.Gr4pmError):
        b.process_bulk(d[:K - 1])
    assert b.output_items(n_in) == samples and b.pending == 0  # nothing was taken
    assert np.array_equal(bits(run(b, v)), bits(one_call(I, V, R, K)))
