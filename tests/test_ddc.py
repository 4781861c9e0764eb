"""The Ddc on the GPU: every output item against the float64 statement of its definition within a derived bound (also
from start indices beyond 2^32); exact properties (call cuts, power-of-two scaling, integer ingest, row stride, reset,
two handles); the identity and the Channelizer's rows; wideband IQ -> Ddc -> NativeMultiChannelReceiver -> payload
bytes; error paths.  The kernel has one form, so there is no fast-against-generic test.

The bound of the float64 tests, per output item:
    |y - y64| <= C * 2^-24 * sum_t |h[t]| * max |x| over the item's L samples,   C = L + 8
L for the sum accumulated in sequence, 8 for the rounding of the rotated taps, the complex products and the rotator with
its product.  First order, worst case: not a fit."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import _ddc_ref as dref
import test_syncword_float64 as t64
from _frontend import (FREQ_POOL, bits, dev, exact_iq_forms, host, load_package, random_taps, received_packets,
                       short_calls_of_mixed_formats)

pytestmark = pytest.mark.gpu

SIZES = [(5, 60, 3), (4, 48, 1), (64, 768, 8), (1, 1, 1), (20, 161, 16), (3, 96, 2), (1000, 2000, 2), (16, 8192, 9)]


def freqs_of(D, L, K):
    o = SIZES.index((D, L, K)) if (D, L, K) in SIZES else 0
    return [FREQ_POOL[(o + k) % len(FREQ_POOL)] for k in range(K)]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def default_taps(pkg, D, L):
    """the default design where L is a multiple of D, else the same design at L taps"""
    if L % D == 0:
        return pkg.ddc_taps(D, L // D)
    return dref.kaiser_taps64(D, L).astype(np.float32)


@functools.lru_cache(maxsize=None)
def base_stream():
    x = t64.dynamic_range_stream()
    x.setflags(write=False)
    return x


def dynamic_stream(D):
    """test_syncword_float64.dynamic_range_stream (segments from 2^-20 to 2^10 and 2^-64, noise, exact zeros, impulses)
    followed by unit impulses at frame offsets 0, 1, D - 1 with silence between them, and an incomplete frame"""
    tail = np.zeros(120 * D + D // 2 + 1, np.complex64)
    for i, off in enumerate((0, 1, D - 1)):
        tail[(5 + 35 * i) * D + off] = 1.0 + 0.5j
    return np.concatenate([base_stream(), tail])


def run(pkg, x, D, freqs, taps, cuts=None, start=0):
    """the stream through one handle in one call, or cut at `cuts`; [K, frames] on the host"""
    import torch
    d = pkg.Ddc(freqs, D, taps=taps, start_index=start, max_frames=max(x.size // D + 1, 1))
    xd = dev(x)
    parts, lo = [], 0
    for hi in list(cuts or []) + [x.size]:
        want = d.output_items(hi - lo)
        parts.append(d.process_bulk(xd[lo:hi]))
        assert parts[-1].shape[1] == want
        lo = hi
    return host(torch.cat(parts, dim=1))


def ratio(y, y64, x, h, D):
    """|y - y64| / (2^-24 sum|h| max|x| over the window); items whose window is all zeros must be exactly zero"""
    wm = dref.window_max(x, D, h.size)
    scale = dref.EPS32 * np.sum(np.abs(h.astype(np.float64))) * wm
    err = np.abs(y.astype(np.complex128) - y64)
    assert np.all(err[:, scale == 0] == 0)
    nz = scale > 0
    return err[:, nz] / scale[nz][None, :]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("D,L,K", SIZES)
def test_against_float64(pkg, D, L, K):
    """every output item within C = L + 8 of the float64 rotated-taps form (pinned to the definition by
    tests/test_ddc_ref.py), the default design and a random prototype.  Measured on MI355X (max / rms of the ratio):
    see DESIGN.md section 16"""
    x = dynamic_stream(D)
    f = freqs_of(D, L, K)
    Cb = L + 8
    for name, h in (("default", default_taps(pkg, D, L)), ("random", random_taps(D, L, 3))):
        y64 = dref.ddc64_rotated(x, h.astype(np.float64), D, f)
        y = run(pkg, x, D, f, h)
        assert y.shape == y64.shape == (K, x.size // D)
        r = ratio(y, y64, x, h, D)
        print(f"\n[ddc float64] D = {D}, L = {L}, K = {K}, {name} taps: max ratio {r.max():.3f}, "
              f"rms {np.sqrt(np.mean(r ** 2)):.4f} (C = {Cb})")
        assert r.max() <= Cb
        if name == "random":  # the stimulus: the 2^10 segment reaches the output (a broadband prototype, any frequency)
            assert np.max(np.abs(y64)) > 50.0


@pytest.mark.timeout(300)
@pytest.mark.parametrize("start", [(1 << 32) - 1000, (1 << 40) + 3])
def test_start_index(pkg, start):
    """a phase computed in float, or one that overflows, does not survive a stream that starts here (the first start
    crosses 2^32 after 1000 samples)"""
    D, L, K = 5, 60, 3
    rng = np.random.default_rng(17)
    n = 4000 * D + 3
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    f = [-0.3137, 3.0 * 2.0 ** -32, 0.123456789]
    h = random_taps(D, L, 4)
    y64 = dref.ddc64_rotated(x, h.astype(np.float64), D, f, start)
    items = [0, 1, 199, 200, 201, 3999]
    direct = dref.ddc64_direct(x, h.astype(np.float64), D, f, start, items)
    assert np.max(np.abs(y64[:, items] - direct)) <= 1e-12 * np.sum(np.abs(h)) * np.max(np.abs(x))
    y = run(pkg, x, D, f, h, cuts=[777, 2 * D * 1000 + 1], start=start)
    r = ratio(y, y64, x, h, D)
    print(f"\n[ddc start_index] start = {start}: max ratio {r.max():.3f}, rms {np.sqrt(np.mean(r ** 2)):.4f} (C = {L + 8})")
    assert r.max() <= L + 8
    # and the start is not ignored
    assert np.max(np.abs(y - dref.ddc64_rotated(x, h.astype(np.float64), D, f, 0))) > 0.1


@pytest.mark.timeout(300)
@pytest.mark.parametrize("D,L,K", [(5, 60, 3), (64, 768, 8), (1000, 2000, 2), (1, 1, 1)])
def test_one_call_equals_any_chain_of_calls(pkg, D, L, K):
    rng = np.random.default_rng(D + L)
    n = 300 * D + D // 2 + 3 if D <= 64 else 40 * D + 5
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    h = random_taps(D, L, 1)
    f = freqs_of(D, L, K)
    one = run(pkg, x, D, f, h, start=12345)
    assert one.shape == (K, n // D)
    steps = [0, 1, D - 1, D, D + 1, L - 1, 0, 0, 1, 1, 2 * D - 1, 3]
    cuts, pos = [], 0
    for s in steps + [int(v) for v in rng.integers(0, 3 * D + 1, 40)] + [int(v) for v in rng.integers(0, 9 * max(L, D), 6)]:
        if pos + s <= n:
            pos += s
            cuts.append(pos)
    assert len(cuts) > 30
    assert np.array_equal(bits(run(pkg, x, D, f, h, cuts, start=12345)), bits(one))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("D,L,K", [(5, 60, 3), (16, 192, 8)])
def test_power_of_two_scaling_is_exact(pkg, D, L, K):
    """input times 2^7 and 2^-9: the output times the same, bit for bit (no denormals anywhere: the stream's
    components are normal or exactly zero and far from the ends of the range)"""
    rng = np.random.default_rng(5)
    n = 200 * D
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    x[50 * D:50 * D + 2 * L] = 0
    h = default_taps(pkg, D, L)
    f = freqs_of(D, L, K)
    y0 = run(pkg, x, D, f, h)
    for k in (7, -9):
        s = np.float32(2.0 ** k)
        xs = (x * s).astype(np.complex64)
        assert np.array_equal(xs / s, x)
        assert np.array_equal(bits(run(pkg, xs, D, f, h)), bits((y0 * s).astype(np.complex64))), k


@pytest.mark.timeout(300)
def test_identity_and_channelizer_row(pkg):
    rng = np.random.default_rng(21)
    x = (rng.standard_normal(5001) + 1j * rng.standard_normal(5001)).astype(np.complex64)
    y = run(pkg, x, 1, [0.0], np.ones(1, np.float32), cuts=[1, 1000])
    assert y.shape == (1, x.size) and np.all(y[0] == x)
    # D = M = 16, f_k = k / 16, the channelizer's taps: the channelizer's rows, each side within its own bound
    M, P = 16, 12
    h = pkg.channelizer_taps(M, P)
    n = 400 * M + 5
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    yd = run(pkg, x, M, [k / M for k in range(M)], h)
    yc = host(pkg.Channelizer(M, taps=h).process_bulk(dev(x)))
    assert yd.shape == yc.shape == (M, n // M)
    bound = ((P * M + 8) + (P + 5 * np.log2(M))) * dref.EPS32 * np.sum(np.abs(h.astype(np.float64)))
    err = np.abs(yd.astype(np.complex128) - yc.astype(np.complex128)) / dref.window_max(x, M, P * M)[None, :]
    print(f"\n[ddc against channelizer] max |difference| / (2^-24 sum|h| max|x|) = "
          f"{err.max() / (dref.EPS32 * np.sum(np.abs(h.astype(np.float64)))):.3f}")
    assert err.max() <= bound


@pytest.mark.timeout(300)
def test_integer_ingest_is_bit_equal(pkg):
    """process_bulk(v) on integer IQ against process_bulk(iq_unpack(v)), default and non-default scale, the formats
    (and complex64) mixed across the calls of one handle"""
    import torch
    D, L, K = 5, 60, 3
    rng = np.random.default_rng(8)
    f = freqs_of(D, L, K)
    h = random_taps(D, L, 6)
    v16 = dev(rng.integers(-32768, 32768, (2003, 2)).astype(np.int16))
    v8 = dev(rng.integers(-128, 128, (1501, 2)).astype(np.int8))
    vu = dev(rng.integers(0, 256, (1777, 2)).astype(np.uint8))
    xc = dev((rng.standard_normal(999) + 1j * rng.standard_normal(999)).astype(np.complex64))
    calls = [(v16, None), (vu, None), (xc, None), (v8, 0.37), (v16, 3.0e-5), (vu[:7], 1.0 / 64), (v8[:4], None), (vu, 0.011)]
    a = pkg.Ddc(f, D, taps=h, start_index=99)
    b = pkg.Ddc(f, D, taps=h, start_index=99)
    n_out = 0
    for v, scale in calls:
        if v.dtype == torch.complex64:
            ya, yb = a.process_bulk(v), b.process_bulk(v)
        else:
            ya = a.process_bulk(v, scale=scale)
            yb = b.process_bulk(pkg.iq_unpack(v, scale=scale))
        assert ya.shape == yb.shape
        assert np.array_equal(bits(host(ya)), bits(host(yb)))
        n_out += ya.shape[1]
    assert n_out == sum(v.shape[0] for v, _ in calls) // D
    # one format alone, one call, from a fresh handle
    for v, scale in ((v16, None), (v8, None), (vu, None), (v16, 0.5)):
        a.reset(), b.reset()
        ya, yb = a.process_bulk(v, scale=scale), b.process_bulk(pkg.iq_unpack(v, scale=scale))
        assert ya.shape[1] == v.shape[0] // D and np.array_equal(bits(host(ya)), bits(host(yb)))
        assert np.max(np.abs(host(ya))) > 0


def test_short_calls_of_mixed_formats_equal_one_call(pkg):
    """the history kernel's hard case: calls of 1, 2, 7, 3, 64, 1, ... samples against a tail of 59 to 63, so that most
    of a new tail comes from the old one and the boundary between the old tail and the call's input falls inside it,
    the calls by turns complex64, sc16, sc8 and cu8 forms that unpack exactly to the stream: bit for bit what one
    complex64 call on a fresh handle gives"""
    D, L, K = 5, 60, 3
    x, forms = exact_iq_forms(624, 31)
    f, h = freqs_of(D, L, K), random_taps(D, L, 7)
    one = run(pkg, x, D, f, h, start=99)
    got = short_calls_of_mixed_formats(pkg, pkg.Ddc(f, D, taps=h, start_index=99), x, forms)
    assert one.shape == got.shape == (K, x.size // D)
    assert np.array_equal(bits(got), bits(one))
    assert np.all(np.max(np.abs(one), axis=1) > 0)


@pytest.mark.timeout(300)
def test_stride_reset_two_handles(pkg):
    import torch
    D, L, K = 5, 60, 3
    rng = np.random.default_rng(9)
    n = 5000 * D + 3
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    h = default_taps(pkg, D, L)
    f = freqs_of(D, L, K)
    full = run(pkg, x, D, f, h, start=7)
    F = n // D
    # a caller's tensor with a larger row stride: the packed result, padding untouched
    fill = np.complex64(complex(np.float32(-7.25), np.float32(3.5)))
    big = torch.full((K, F + 45), complex(fill), dtype=torch.complex64, device="cuda")
    d = pkg.Ddc(f, D, taps=h, start_index=7)
    y = d.process_bulk(dev(x), out=big[:, 5:5 + F + 3])
    assert tuple(y.shape) == (K, F)
    b = host(big)
    assert np.array_equal(bits(b[:, 5:5 + F]), bits(full))
    assert np.all(b[:, :5] == fill) and np.all(b[:, 5 + F:] == fill)
    # reset(): the stream from start_index again (the handle above has seen x and carries 3 samples)
    d.reset()
    assert d.output_items(D - 1) == 0 and d.output_items(D) == 1
    assert np.array_equal(bits(host(d.process_bulk(dev(x)))), bits(full))
    # frequencies: w / 2^32 folded to [-0.5, 0.5)
    assert d.frequencies.dtype == np.float64
    assert d.frequencies.tolist() == [dref.quantised(v) for v in f]
    q = pkg.Ddc([0.5, -0.25, 3.0 * 2.0 ** -32, 1.75, 0.1], D).frequencies.tolist()
    assert q == [-0.5, -0.25, 3.0 * 2.0 ** -32, -0.25, dref.frequency_word(0.1) / 2.0 ** 32]
    # two handles on two streams at once: what each gives alone
    x2 = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    f2 = [0.2, -0.44, 0.01]
    full2 = run(pkg, x2, D, f2, h)
    xa, xb = dev(x), dev(x2)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        c1 = pkg.Ddc(f, D, taps=h, start_index=7)
    with torch.cuda.stream(s2):
        c2 = pkg.Ddc(f2, D, taps=h)
    p1, p2, lo = [], [], 0
    for hi in (1000, 1001, 9000, 20000, n):
        with torch.cuda.stream(s1):
            p1.append(c1.process_bulk(xa[lo:hi]))
        with torch.cuda.stream(s2):
            p2.append(c2.process_bulk(xb[lo:hi]))
        lo = hi
    torch.cuda.synchronize()
    assert np.array_equal(bits(host(torch.cat(p1, dim=1))), bits(full))
    assert np.array_equal(bits(host(torch.cat(p2, dim=1))), bits(full2))


@pytest.mark.timeout(600)
def test_wideband_to_packets_end_to_end(pkg):
    """D = 5, four carriers at -0.37, -0.11, +0.13, +0.41 cycles per sample (on no power-of-two grid; neighbours at
    least 0.22 apart), each with three bursts of distinct random payloads from PacketTransmitter and a CFO of its own,
    noise of sigma 0.05 on the wideband stream, synthesised on the GPU in complex128 (zero-stuff by D, filter with D h,
    mix with the quantised frequency in integer phases); Ddc (four unequal calls) -> NativeMultiChannelReceiver: per row
    as many detector tags as bursts, each within one item of where the same receiver finds them in the float64
    reference's output.  Every row through NativePacketReceiver: every payload byte for byte.  syncword_threshold is
    20.0 as in tests/test_channelizer.py.  The noise seed is 5, the first one tried."""
    import torch
    D, P, N = 5, 12, 30000
    carriers = [-0.37, -0.11, 0.13, 0.41]
    K = len(carriers)
    rng = np.random.default_rng(2026)
    h = pkg.ddc_taps(D, P)
    hd = torch.from_numpy(h.astype(np.float64)).cuda().reshape(P, D) * D
    tx = pkg.PacketTransmitter()
    i = torch.arange(N * D, device="cuda", dtype=torch.int64)
    x = torch.zeros(N * D, dtype=torch.complex128, device="cuda")
    sent = []
    for f in carriers:
        payloads = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(30, 200, 3)]
        gaps = [int(g) for g in rng.integers(2500, 4000, 3)]
        tx.reset()
        v, _, _ = tx.process_bulk(payloads, gaps=gaps)
        assert v.numel() + 9000 < N
        cfo = float(rng.uniform(-0.03, 0.03))  # rad / item; the detector's +-4 bins reach +-0.042
        v = v.to(torch.complex128) * torch.exp(1j * cfo * torch.arange(v.numel(), device="cuda", dtype=torch.float64))
        vp = torch.zeros(N + P - 1, dtype=torch.complex128, device="cuda")
        vp[P - 1:P - 1 + v.numel()] = v
        s = torch.zeros((N, D), dtype=torch.complex128, device="cuda")
        for p in range(P):  # zero-stuff by D and filter with D h: sample n D + r takes h[p D + r] v[n - p]
            s += hd[p][None, :] * vp[P - 1 - p:P - 1 - p + N, None]
        phi = (dref.frequency_word(f) * i) & 0xFFFFFFFF  # w i < 2^50: exact in int64
        x += s.reshape(-1) * torch.exp(2j * np.pi * (phi.to(torch.float64) / 4294967296.0))
        sent.append(payloads)
    g = torch.Generator(device="cuda").manual_seed(5)
    noise = torch.randn((N * D, 2), dtype=torch.float64, device="cuda", generator=g)
    x = x + (0.05 / np.sqrt(2.0)) * torch.view_as_complex(noise)
    x32 = x.to(torch.complex64).contiguous()
    torch.cuda.synchronize()

    d = pkg.Ddc(carriers, D, taps=h)
    assert d.frequencies.tolist() == [dref.quantised(f) for f in carriers]
    parts, lo = [], 0
    for hi in (D * 7000 + 3, D * 7000 + 4, D * 19000 - 1, N * D):
        parts.append(d.process_bulk(x32[lo:hi]))
        lo = hi
    y = torch.cat(parts, dim=1).contiguous()
    assert tuple(y.shape) == (K, N)
    y64 = dref.ddc64_rotated(host(x32), h.astype(np.float64), D, carriers).astype(np.complex64)
    yr = dev(y64)

    got = pkg.NativeMultiChannelReceiver(K, syncword_threshold=20.0, max_items=N).process_bulk(y)
    ref = pkg.NativeMultiChannelReceiver(K, syncword_threshold=20.0, max_items=N).process_bulk(yr)
    for k in range(K):
        a, b = got[k]["detector_tags"]["index"].astype(np.int64), ref[k]["detector_tags"]["index"].astype(np.int64)
        print(f"\n[ddc end to end] row {k}: tags at {a.tolist()}, in the float64 reference's output at {b.tolist()}")
        assert a.size == len(sent[k]) and b.size == len(sent[k]), (k, a, b)
        assert np.all(np.abs(a - b) <= 1), (k, a, b)
    for k in range(K):
        rx = pkg.NativePacketReceiver(max_items=N, tags_cap=2048, syncword_threshold=20.0, decode_headers=True,
                                      packets_only=True)
        assert received_packets(rx.process_bulk(y[k].contiguous())) == sent[k], k


def test_error_paths_return_statuses(pkg):
    import torch
    L = pkg.lib()
    abi = importlib.import_module(pkg.__name__ + "._abi")
    D, K = 5, 3
    fr = (C.c_double * 65)(*([0.1] * 65))
    tp = (C.c_float * 8193)(*([0.01] * 8193))

    def create(n_channels=K, decimation=D, frequencies=fr, taps=tp, n_taps=60, max_frames=100, start_index=0):
        p = abi.DdcParams(n_channels, decimation, C.cast(frequencies, C.c_void_p), C.cast(taps, C.c_void_p), n_taps,
                          max_frames, start_index, None)
        h = C.c_void_p(0x1234)
        st = L.gr4pm_ddc_create(C.byref(p), C.byref(h))
        if st == 0:
            L.gr4pm_ddc_destroy(h)
        else:
            assert not h.value and L.gr4pm_last_error()
        return st

    assert create() == 0
    assert create(taps=None, n_taps=0) == 0  # the default design
    assert create(n_taps=8192, decimation=1024) == 0
    assert create(n_channels=64) == 0
    for bad in (dict(n_channels=0), dict(n_channels=65), dict(decimation=0), dict(decimation=1025), dict(n_taps=0),
                dict(n_taps=8193), dict(frequencies=None), dict(max_frames=0)):
        assert create(**bad) == -1, bad
    for v in (float("nan"), float("inf"), -float("inf")):
        bad_f = (C.c_double * 3)(0.1, 0.2, v)
        assert create(frequencies=bad_f) == -1 and b"finite" in L.gr4pm_last_error()
    assert L.gr4pm_ddc_create(None, None) == -1
    with pytest.raises(pkg.Gr4pmError):
        pkg.Ddc([0.1], 5, taps=[])
    with pytest.raises(pkg.Gr4pmError):
        pkg.Ddc([], 5)
    with pytest.raises(pkg.Gr4pmError):
        pkg.Ddc([0.1, float("nan")], 5)

    d = pkg.Ddc([0.1, -0.2, 0.3], D, taps_per_phase=12, max_frames=100, start_index=5)
    x = torch.randn(101 * D, dtype=torch.complex64, device="cuda")
    out = torch.zeros((K, 128), dtype=torch.complex64, device="cuda")
    n = C.c_size_t(7)
    st = L.gr4pm_ddc_process(d._h, x.data_ptr(), 101 * D, out.data_ptr(), 128, 128, C.byref(n))
    assert st == -5 and n.value == 0 and b"made for" in L.gr4pm_last_error()       # beyond max_frames D
    n = C.c_size_t(7)
    st = L.gr4pm_ddc_process(d._h, x.data_ptr(), 50 * D, out.data_ptr(), 128, 49, C.byref(n))
    assert st == -5 and n.value == 0                                                  # out_cap_frames too small
    for args in ((None, 50 * D, out.data_ptr(), 128, 128), (x.data_ptr(), 50 * D, None, 128, 128),
                 (x.data_ptr(), 50 * D, out.data_ptr(), 10, 128)):                    # null pointers, out_stride < frames
        n = C.c_size_t(7)
        assert L.gr4pm_ddc_process(d._h, *args, C.byref(n)) == -1 and n.value == 0
    assert L.gr4pm_ddc_process(d._h, x.data_ptr(), 50 * D, out.data_ptr(), 128, 128, None) == -1
    assert L.gr4pm_ddc_process(None, x.data_ptr(), 50 * D, out.data_ptr(), 128, 128, C.byref(n)) == -1
    n = C.c_size_t(7)
    assert L.gr4pm_ddc_process_iq(d._h, x.data_ptr(), 9, 0.0, 50 * D, out.data_ptr(), 128, 128, C.byref(n)) == -1
    assert n.value == 0 and b"format" in L.gr4pm_last_error()
    assert L.gr4pm_ddc_frequencies(d._h, None) == -1 and L.gr4pm_ddc_output_items(d._h, 5, None) == -1
    with pytest.raises(pkg.Gr4pmError):
        d.process_bulk(x)
    with pytest.raises(pkg.Gr4pmError):
        d.process_bulk(x[:50 * D], out=out[:, :49])
    # none of the refused calls moved the stream or wrote anything: the handle still is at its start
    assert d.output_items(D - 1) == 0
    assert np.all(host(out) == 0)
    y = d.process_bulk(x[:50 * D], out=out)
    assert tuple(y.shape) == (K, 50)
    fresh = pkg.Ddc([0.1, -0.2, 0.3], D, taps_per_phase=12, start_index=5).process_bulk(x[:50 * D])
    assert np.array_equal(bits(host(y)), bits(host(fresh)))
    assert d.process_bulk(x[:0]).shape[1] == 0
