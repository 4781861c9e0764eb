"""The FftDdc block on the GPU against the float64 statement of its definition (tests/_fft_ddc_ref.py) within the derived
first-order bound (device_bound there), and its exact properties: the same bits under any cutting
of the stream into calls, integer ingest, reset, zeros in giving zeros out, short calls, refusals.

Shapes: n = 5 hop + 77 samples at the (D, V, R, K) of tests/test_fft_ddc_ref.py's DEVICE_CASES, with its stimulus, taps and
frequencies (both sides of a 64-bin boundary, on a bin, half-way between bins, a slice across +-0.5).

Measured on MI355X, worst error over bound per case, in DEVICE_CASES' order: 0.0006, 0.0028, 0.0018, 0.0010, 0.0081."""
import ctypes as C
import functools

import numpy as np
import pytest

import _fft_ddc_ref as fref
import test_fft_ddc_ref as cpu
from _frontend import bits, dev, exact_iq_forms, host, load_package

pytestmark = pytest.mark.gpu

N = fref.N
START = cpu.START
CASES = cpu.DEVICE_CASES


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@functools.lru_cache(maxsize=None)
def setting(D, V, R, K):
    """(x complex64, taps float32, frequencies, the float64 reference, the bound), computed once per case"""
    hop = N - V
    x = cpu.stimulus(5 * hop + 77).astype(np.complex64)
    h = cpu.taps_for(D, V).astype(np.float32)
    f = cpu.device_freqs(K)
    want = fref.fft_ddc64(x, h, D, f, V=V, R=R, start=START)
    bound = fref.device_bound(x, h, D, f, V, R)
    for a in (x, h, want, bound):
        a.setflags(write=False)
    return x, h, f, want, bound


def make(pkg, D, V, R, K, start=START):
    _, h, f, _, _ = setting(D, V, R, K)
    return pkg.FftDdc(f, D, taps=h, overlap=V, images=R, start_index=start)


def run(block, x, cuts=(), scale=None):
    """x through the block in calls of the lengths `cuts`, then the rest; the rows joined, on the host"""
    import torch
    d, lo, parts = dev(x), 0, []
    for c in list(cuts) + [len(x)]:
        if lo >= len(x) and parts:
            break
        part = d[lo:lo + c]
        assert block.frames_for(part.shape[0]) >= 0
        want = block.frames_for(part.shape[0])
        y = block.process_bulk(part, scale=scale) if scale is not None else block.process_bulk(part)
        assert y.shape[1] == want
        parts.append(y)
        lo += c
    return host(torch.cat(parts, dim=1))


@functools.lru_cache(maxsize=None)
def one_call(D, V, R, K):
    out = run(make(load_package(), D, V, R, K), setting(D, V, R, K)[0])
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("D,V,R,K", CASES)
def test_against_float64(pkg, D, V, R, K):
    _, _, f, want, bound = setting(D, V, R, K)
    b = make(pkg, D, V, R, K)
    assert (b.hop, b.overlap) == (N - V, V)
    assert np.array_equal(b.frequencies, [fref.frequency_word(v) / 2.0 ** 32 - (fref.frequency_word(v) >= 1 << 31) for v in f])
    got = one_call(D, V, R, K)
    assert got.shape == want.shape == (K, 5 * (N - V) // D)
    err = np.abs(got.astype(np.complex128) - want)
    print(f"D {D} V {V} R {R} K {K}: worst error / bound {np.max(err / bound):.4f}, worst error {np.max(err):.3e} "
          f"of {np.max(np.abs(want)):.3f}")
    assert np.all(np.isfinite(got.view(np.float32)))
    assert np.all(err <= bound)


@pytest.mark.parametrize("D,V,R,K", CASES)
def test_call_cuts_give_the_same_bits(pkg, D, V, R, K):
    x = setting(D, V, R, K)[0]
    hop = N - V
    first = hop + D - 1  # samples that complete segment 0
    rng = np.random.default_rng(D + K)
    # inside the first V samples, then single samples across the end of segment 0, then across the end of segment 1
    cuts = [3, max(V // 2, 1), first - 3 - max(V // 2, 1) - 2, 1, 1, 1, 1, hop - 4, 1, 1] + [int(c) for c in rng.integers(1, 2 * hop, 6)]
    assert min(cuts) >= 1 and cuts[0] + cuts[1] < max(V, 5)
    got = run(make(pkg, D, V, R, K), x, cuts)
    assert np.array_equal(bits(got), bits(one_call(D, V, R, K)))


@pytest.mark.parametrize("D,V,R,K", [CASES[1], CASES[3]])
def test_integer_iq_is_unpack_then_process(pkg, D, V, R, K):
    hop = N - V
    n = 3 * hop + 77
    _, forms = exact_iq_forms(n, 9)
    for a, scale in forms[1:]:
        unpacked = host(pkg.iq_unpack(dev(a), scale))
        want = run(make(pkg, D, V, R, K), unpacked)
        got = run(make(pkg, D, V, R, K), a, cuts=(hop // 3, hop + 5), scale=scale if scale is not None else None)
        assert want.shape[1] == 3 * hop // D
        assert np.array_equal(bits(got), bits(want)), a.dtype


def test_reset_reproduces_the_first_run(pkg):
    D, V, R, K = CASES[1]
    x = setting(D, V, R, K)[0]
    b = make(pkg, D, V, R, K)
    first = run(b, x, cuts=(1000,))
    b.reset()
    again = run(b, x, cuts=(N - V + 3, 17))
    assert np.array_equal(bits(first), bits(again)) and np.array_equal(bits(first), bits(one_call(D, V, R, K)))


@pytest.mark.parametrize("D,V,R,K", [CASES[0], CASES[2]])
def test_a_window_of_zeros_gives_exact_zeros(pkg, D, V, R, K):
    hop = N - V
    x = np.array(setting(D, V, R, K)[0])
    lo, hi = hop + 100, hop + 100 + N + hop  # at least one segment begins in [lo, hi - N]; the last one ends behind hi
    x[lo:hi] = 0
    got = run(make(pkg, D, V, R, K), x)
    zero_segments = [s for s in range(5) if s * hop - V + D - 1 >= lo and s * hop - V + D - 1 + N <= hi]
    assert len(zero_segments) >= 1
    fr = hop // D
    for s in zero_segments:
        assert not np.any(got[:, s * fr:(s + 1) * fr].view(np.float32)), s
    assert np.any(got[:, :fr]) and np.any(got[:, -fr:])


def test_a_call_shorter_than_a_hop_yields_nothing_and_the_next_completes(pkg):
    D, V, R, K = CASES[1]
    x = setting(D, V, R, K)[0]
    hop = N - V
    b = make(pkg, D, V, R, K)
    assert b.frames_for(hop // 2) == 0
    y = b.process_bulk(dev(x[:hop // 2]))
    assert tuple(y.shape) == (K, 0)
    assert b.frames_for(hop) == hop // D
    rest = run(b, x[hop // 2:], cuts=(hop,))
    assert np.array_equal(bits(rest), bits(one_call(D, V, R, K)))


def test_refusals_leave_the_handle_usable(pkg):
    import torch
    from gr4_packet_modem_amd import _abi
    L = pkg.lib()
    D, V, R, K = CASES[1]
    x, h, f, _, _ = setting(D, V, R, K)
    nan_taps, inf_taps = np.array(h), np.array(h)
    nan_taps[7], inf_taps[0] = np.nan, np.inf
    ok = dict(frequencies=f, decimation=D, taps=h, overlap=V, images=R)
    for bad in (dict(decimation=5), dict(decimation=2), dict(decimation=128), dict(images=3), dict(images=0), dict(images=2 * D),
                dict(overlap=V + 1), dict(overlap=(h.size - 2) // D * D), dict(overlap=N - 64 + D), dict(frequencies=[]),
                dict(frequencies=[0.01] * 65), dict(frequencies=[0.1, np.nan]), dict(frequencies=[np.inf]), dict(taps=nan_taps),
                dict(taps=inf_taps)):
        with pytest.raises(pkg.Gr4pmError):
            pkg.FftDdc(**{**ok, **bad})
    # NULL arrays at create
    fa = np.asarray(f, dtype=np.float64)
    for freqs in (None, fa.ctypes.data_as(C.c_void_p)):
        hd = C.c_void_p(0x1234)
        p = _abi.FftDdcParams(K, D, freqs, h.ctypes.data_as(C.c_void_p), h.size if freqs is None else 0, 12, V, R, 0, None)
        assert L.gr4pm_fft_ddc_create(C.byref(p), C.byref(hd)) == -1  # no frequencies; a prototype of 0 taps
        assert hd.value is None

    b = make(pkg, D, V, R, K)
    d = dev(x)
    frames = b.frames_for(x.size)
    out = torch.empty((K, frames), dtype=torch.complex64, device="cuda")
    n = C.c_size_t(77)
    call = lambda inp, n_in, o, stride, cap: L.gr4pm_fft_ddc_process(b._h, inp, n_in, o, stride, cap, C.byref(n))
    assert call(None, x.size, out.data_ptr(), frames, frames) == -1 and n.value == 0          # no input
    assert call(d.data_ptr(), x.size, None, frames, frames) == -1 and n.value == 0            # no output
    assert call(d.data_ptr(), x.size, out.data_ptr(), frames - 1, frames) == -1 and n.value == 0  # a stride below the frames
    assert call(d.data_ptr(), x.size, out.data_ptr(), frames, frames - 1) == -5 and n.value == 0  # no room
    assert call(d.data_ptr(), (1 << 40) + 1, out.data_ptr(), frames, frames) == -5 and n.value == 0  # 2^40 samples a call
    assert L.gr4pm_fft_ddc_process_iq(b._h, d.data_ptr(), 9, 0.0, x.size, out.data_ptr(), frames, frames, C.byref(n)) == -1
    with pytest.raises(pkg.Gr4pmError):
        b.frames_for((1 << 40) + 1)
    with pytest.raises(pkg.Gr4pmError):
        b.process_bulk(d, out=out[:, :frames - 1])
    assert b.frames_for(x.size) == frames  # nothing was taken
    assert np.array_equal(bits(run(b, x)), bits(one_call(D, V, R, K)))
