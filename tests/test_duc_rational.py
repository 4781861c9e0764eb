"""The Duc resampling by I / D on the GPU (gr4pm_duc_create_rational): every output sample against
the float64 statement of its definition within a derived bound (also from start indices beyond 2^32); exact properties
(decimation = 1 is the integer Duc, one row at f = 0 is every D-th sample of the integer Duc, call cuts, power-of-two
scaling, a start that moves no phase, row stride, reset, two handles); PacketTransmitter -> Duc(25 / 4) -> Ddc(4 / 25)
-> receivers -> payload bytes, and the two file apps on an sc16 file at 25 / 4 of the modem's rate; error paths.

The bound of the float64 tests, per output sample j (newest item m_j, branch r_j):
    |x - x64| <= C * 2^-24 * S[j],   S[j] = sum_k |a_k| (sum_p |h[p I + r_j]|) max_p |v_k[m_j - p]|,   C = 2 P + 3 K + 8
sqrt(2) P for the filter's sequential sum (one rounding per fmaf and component, real taps), 2 sqrt(2) K for the mix's
sum (two roundings per component and row), 8 for the rounding of the taps, of the rotator's two factors and of their
product (1 + 1 + 1 + 2 sqrt(2) < 6).  First order, worst case: not a fit (DESIGN.md section 19 has the derivation).

Shapes are (I, D, L, K).  The default design's band edges are in units of the input rate and refused beyond half of the
output rate, so the shapes with I < D take the design at edges scaled by I / D."""
import ctypes as C
import importlib
import importlib.util
import os

import numpy as np
import pytest

import _ddc_ref as dref
import _duc_rational_ref as rref
from _frontend import FREQ_POOL, bits, dev, host, load_package, random_taps, received_packets
from test_duc import dynamic_rows, gains_of

pytestmark = pytest.mark.gpu

SIZES = [(25, 4, 300, 3), (3, 2, 24, 1), (12, 5, 61, 2), (1, 7, 30, 1), (5, 3, 3, 2), (1000, 63, 2000, 2),
         (63, 64, 768, 16), (1023, 64, 8192, 9), (2, 3, 24, 64)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def freqs_of(I, D, L, K):
    o = SIZES.index((I, D, L, K)) if (I, D, L, K) in SIZES else 0
    return [FREQ_POOL[(o + k) % len(FREQ_POOL)] for k in range(K)]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def default_taps(pkg, I, D, L):
    """the default design (band edges scaled by I / D where I < D) where L is a multiple of I, else the same design at
    L taps"""
    m = min(1.0, I / D)
    if L % I == 0:
        return pkg.duc_rational_taps(I, D, L // I, 0.25 * m, 0.75 * m)
    return rref.rational_taps64(I, D, L, 0.25 * m, 0.75 * m).astype(np.float32)


def items_of(I, D, L):
    """at least 40 P items and 20000 samples, so that every shape has several tiles and crosses aligned blocks"""
    P = -(-L // I)
    return max(40 * P, 3000, -(-20000 * D // I))


def run(pkg, v, I, D, freqs, taps, gains=None, cuts=None, start=0):
    """the rows through one handle in one call, or cut at `cuts` (item positions); [ceil(n I / D)] on the host.
    output_items is exact before each call"""
    import torch
    d = pkg.Duc(freqs, I, decimation=D, gains=gains, taps=taps, start_index=start, max_items=max(v.shape[1], 1))
    assert (d.interpolation, d.decimation) == (I, D) and d.rate * D == I
    vd = dev(v)
    parts, lo = [], 0
    for hi in list(cuts or []) + [v.shape[1]]:
        want = d.output_items(hi - lo)
        assert want == rref.sample_count(hi, I, D) - rref.sample_count(lo, I, D)
        parts.append(d.process_bulk(vd[:, lo:hi]))
        assert parts[-1].shape == (want,)
        lo = hi
    return host(torch.cat(parts))


def ratio(x, x64, v, h, I, D, gains):
    """|x - x64| / (2^-24 S); samples with S = 0 (a window of zeros, or a branch without taps) must be exactly zero"""
    S = rref.window_scale(v, h.astype(np.float64), I, D, gains)
    err = np.abs(x.astype(np.complex128) - x64)
    assert np.all(x[S == 0] == 0)
    nz = S > 0
    return err[nz] / (rref.EPS32 * S[nz])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("I,D,L,K", SIZES)
def test_against_float64(pkg, I, D, L, K):
    """every output sample within C = 2 P + 3 K + 8 of the float64 form (pinned to the definition by
    tests/test_duc_rational_ref.py), the default design and a random-sign prototype.  Max / rms of the ratio as
    measured on MI355X: DESIGN.md section 19's accuracy table"""
    P = -(-L // I)
    n = items_of(I, D, L)
    v = dynamic_rows(K, n, P)
    f, a = freqs_of(I, D, L, K), gains_of(K)
    Cb = 2 * P + 3 * K + 8
    for name, h in (("default", default_taps(pkg, I, D, L)), ("random", random_taps(I, L, 3))):
        x64 = rref.rduc64_form(v, h.astype(np.float64), I, D, f, a)
        x = run(pkg, v, I, D, f, h, a)
        assert x.shape == x64.shape == (rref.sample_count(n, I, D),)
        r = ratio(x, x64, v, h, I, D, a)
        print(f"\n[rational duc float64] I = {I}, D = {D}, L = {L}, K = {K}, {name} taps: max ratio {r.max():.3f}, "
              f"rms {np.sqrt(np.mean(r ** 2)):.4f} (C = {Cb})")
        assert r.max() <= Cb
        if name == "random":  # the stimulus: the 2^10 segment reaches the output
            assert np.max(np.abs(x64)) > 50.0
        if L < I:  # branches L .. I - 1 have no tap: exact zeros between samples that are not
            _, br = rref.samples(n, I, D)
            assert np.all(x[br >= L] == 0) and np.any(br >= L) and np.max(np.abs(x)) > 0


@pytest.mark.timeout(300)
@pytest.mark.parametrize("start", [(1 << 32) - 1000, (1 << 40) + 3])
def test_start_index(pkg, start):
    """a phase computed in float, or one that overflows, does not survive a stream that starts here (the first start
    crosses 2^32 at output sample 1000)"""
    I, D, L, K = 25, 4, 300, 3
    P = L // I
    rng = np.random.default_rng(17)
    n = 1500
    v = (rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))).astype(np.complex64)
    f = [-0.3137, 3.0 * 2.0 ** -32, 0.123456789]
    a = gains_of(K)
    h = random_taps(I, L, 4)
    x64 = rref.rduc64_form(v, h.astype(np.float64), I, D, f, a, start)
    F = rref.sample_count(n, I, D)
    which = [0, 1, 5, 997, 998, 999, 1000, 1001, 1002, 1023, 1024, 1025, F - 1]
    direct = rref.rduc64_direct(v, h.astype(np.float64), I, D, f, a, start, which)
    S = rref.window_scale(v, h.astype(np.float64), I, D, a)
    assert np.all(np.abs(x64[which] - direct) <= 1e-12 * S[which])
    x = run(pkg, v, I, D, f, h, a, cuts=[155, 901], start=start)
    Cb = 2 * P + 3 * K + 8
    r = ratio(x, x64, v, h, I, D, a)
    print(f"\n[rational duc start_index] start = {start}: max ratio {r.max():.3f}, rms {np.sqrt(np.mean(r ** 2)):.4f} (C = {Cb})")
    assert r.max() <= Cb
    assert np.all(np.abs(x[which] - direct) <= Cb * rref.EPS32 * S[which])
    # and the start is not ignored
    assert np.max(np.abs(x - rref.rduc64_form(v, h.astype(np.float64), I, D, f, a, 0))) > 0.1


def rational_handle(pkg, f, I, D, gains=None, taps=None, start=0, max_items=1 << 20):
    """gr4pm_duc_create_rational by hand: (status, handle)"""
    abi = importlib.import_module(pkg.__name__ + "._abi")
    fr = (C.c_double * max(len(f), 1))(*f)
    ga = None if gains is None else (C.c_double * len(gains))(*gains)
    tp = None if taps is None else np.ascontiguousarray(taps, np.float32)
    p = abi.DucRationalParams(len(f), I, C.cast(fr, C.c_void_p), None if ga is None else C.cast(ga, C.c_void_p),
                              None if tp is None else tp.ctypes.data, 0 if tp is None else tp.size, max_items, start, None, D)
    h = C.c_void_p(0x1234)
    return pkg.lib().gr4pm_duc_create_rational(C.byref(p), C.byref(h)), h


@pytest.mark.parametrize("I,L,K", [(5, 60, 3), (64, 768, 8)])
def test_decimation_one_through_create_rational(pkg, I, L, K):
    import torch
    lib = pkg.lib()
    rng = np.random.default_rng(I)
    n = 1203
    v = dev((rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))).astype(np.complex64))
    f = [FREQ_POOL[(1 + k) % len(FREQ_POOL)] for k in range(K)]
    a = gains_of(K)
    st, h = rational_handle(pkg, f, I, 1, gains=a, start=77)
    assert st == 0 and h.value
    try:
        got_n = C.c_size_t(0)
        assert lib.gr4pm_duc_output_items(h, n, C.byref(got_n)) == 0 and got_n.value == n * I
        out = torch.zeros(n * I, dtype=torch.complex64, device="cuda")
        assert lib.gr4pm_duc_process(h, v.data_ptr(), v.stride(0), n, out.data_ptr(), n * I, C.byref(got_n)) == 0
        assert got_n.value == n * I
        want = pkg.Duc(f, I, gains=a, start_index=77)
        assert want.taps.size == L
        assert np.array_equal(bits(host(out)), bits(host(want.process_bulk(v))))
        assert np.max(np.abs(host(out))) > 0
    finally:
        lib.gr4pm_duc_destroy(h)
    # and through the class: decimation = 1 is the default's handle
    d1 = pkg.Duc(f, I, decimation=1, gains=a, start_index=77)
    assert d1.rate == I and np.array_equal(bits(host(d1.process_bulk(v))), bits(host(out)))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("I,D,L", [(25, 4, 300), (12, 5, 61)])
def test_one_row_at_zero_frequency_is_every_dth_sample_of_the_integer_duc(pkg, I, D, L):
    """K = 1, f = 0 and a gain that is no power of two: sample j equals sample j D of Duc([0], I) on the same row, as
    values (-0 equals +0).  phi = 0 makes the integer Duc's rotated taps real (fl(a h), +-0) and its rotator exactly 1,
    so its extra fmaf add +-0 and its sums are the new filter loop's; here the rotator is (1, 0) as well."""
    rng = np.random.default_rng(I * D)
    n = 2000
    v = (rng.standard_normal((1, n)) + 1j * rng.standard_normal((1, n))).astype(np.complex64)
    v[:, 700:700 + 3 * (L // I)] = 0
    h = random_taps(I, L, 5)
    for gain, start in ((0.75, 0), (-1.25, 1 << 33)):
        x = run(pkg, v, I, D, [0.0], h, gains=[gain], cuts=[3, 1001], start=start)
        full = host(pkg.Duc([0.0], I, gains=[gain], taps=h, max_items=n).process_bulk(dev(v)))
        assert x.shape == full[::D].shape
        assert np.array_equal(x, full[::D])
        assert np.max(np.abs(x)) > 1.0 and np.any(x == 0)


def random_cuts(rng, n, I, D, L):
    """runs of 1-item calls, empty calls, calls that make no sample (I < D) or several per item (I > D), random ones"""
    P = -(-L // I)
    steps = [0, 1, 1, 1, 1, 1, 1, 1, 0, 0, 2, D - 1, D, D + 1, P - 1, P, 1, 1, 1, 2 * D - 1, 3]
    steps += [int(t) for t in rng.integers(0, 3 * D + 1, 40)] + [int(t) for t in rng.integers(0, 9 * max(P, D), 6)]
    cuts, pos = [], 0
    for s in steps:
        if pos + s <= n:
            pos += s
            cuts.append(pos)
    return cuts


@pytest.mark.timeout(300)
@pytest.mark.parametrize("I,D,L,K", [(25, 4, 300, 3), (2, 3, 24, 64), (1000, 63, 2000, 2), (1, 7, 30, 1)])
def test_one_call_equals_any_chain_of_calls(pkg, I, D, L, K):
    """1-item calls, calls that make no sample, several samples per item, and cuts inside and across the rotator's
    aligned blocks of 1024 samples (the start, 12251, is 37 samples short of one)"""
    rng = np.random.default_rng(I + D + L)
    n = max(600, -(-5000 * D // I), 100 * D)  # room for the cuts below
    v = (rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))).astype(np.complex64)
    h = random_taps(I, L, 1)
    f, a = freqs_of(I, D, L, K), gains_of(K)
    one = run(pkg, v, I, D, f, h, a, start=12251)
    assert one.shape == (rref.sample_count(n, I, D),)
    cuts = random_cuts(rng, n, I, D, L)
    assert len(cuts) > 30
    per_call = np.diff([0] + cuts)
    made = np.diff([0] + [rref.sample_count(c, I, D) for c in cuts])
    assert I >= D or np.any((per_call > 0) & (made == 0))
    assert I <= D or np.any(made > per_call)
    edges = (12251 + np.cumsum(made)) // 1024
    assert np.any(np.diff(edges) > 0) and np.any((12251 + np.cumsum(made)) % 1024 != 0)
    assert np.array_equal(bits(run(pkg, v, I, D, f, h, a, cuts, start=12251)), bits(one))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("I,D,L,K", [(25, 4, 300, 3), (12, 5, 61, 2)])
def test_power_of_two_scaling_is_exact(pkg, I, D, L, K):
    """rows times 2^7 and 2^-9: the output times the same, bit for bit (no denormals anywhere); gains of 2^e: the bits
    of scaling row k by 2^e"""
    rng = np.random.default_rng(5)
    n = 1200
    P = -(-L // I)
    v = (rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))).astype(np.complex64)
    v[:, 300:300 + 2 * P] = 0
    h = default_taps(pkg, I, D, L)
    f = freqs_of(I, D, L, K)
    x0 = run(pkg, v, I, D, f, h)
    assert np.max(np.abs(x0)) > 1.0
    for k in (7, -9):
        s = np.float32(2.0 ** k)
        vs = (v * s).astype(np.complex64)
        assert np.array_equal(vs / s, v)
        assert np.array_equal(bits(run(pkg, vs, I, D, f, h)), bits((x0 * s).astype(np.complex64))), k
    e = [(-1.0) ** k * 2.0 ** ((3 * k) % 7 - 3) for k in range(K)]
    ve = (v * np.asarray(e, np.float32)[:, None]).astype(np.complex64)
    assert np.array_equal(bits(run(pkg, v, I, D, f, h, gains=e)), bits(run(pkg, ve, I, D, f, h)))


def test_start_index_that_moves_no_phase_is_bit_equal(pkg):
    """frequency words that are multiples of 2^20 and a start of 2^40 + 4096: every w (start mod 2^32) is a multiple
    of 2^32 and the start a multiple of the rotator's block, so the handle gives what one started at 0 gives"""
    I, D, L = 25, 4, 300
    rng = np.random.default_rng(18)
    n = 900
    v = (rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))).astype(np.complex64)
    f = [3 * 2.0 ** -12, -1000 * 2.0 ** -12, 2047 * 2.0 ** -12]
    assert all(rref.frequency_word(t) % (1 << 20) == 0 and rref.frequency_word(t) for t in f)
    h = random_taps(I, L, 4)
    a = run(pkg, v, I, D, f, h, start=0)
    b = run(pkg, v, I, D, f, h, cuts=[234], start=(1 << 40) + 4096)
    assert np.array_equal(bits(a), bits(b)) and np.max(np.abs(a)) > 0
    assert not np.array_equal(bits(a), bits(run(pkg, v, I, D, f, h, start=(1 << 40) + 4097)))


@pytest.mark.timeout(300)
def test_stride_reset_two_handles(pkg):
    import torch
    I, D, L, K = 25, 4, 300, 3
    rng = np.random.default_rng(9)
    n = 2003
    v = (rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))).astype(np.complex64)
    h = default_taps(pkg, I, D, L)
    f, a = freqs_of(I, D, L, K), gains_of(K)
    full = run(pkg, v, I, D, f, h, a, start=7)
    F = rref.sample_count(n, I, D)
    # rows as a window of a wider tensor, at an odd item offset; the result into a caller's tensor at an odd offset
    # (8-byte aligned only), room to spare untouched
    wide = torch.full((K, n + 45), 3.0 - 2.0j, dtype=torch.complex64, device="cuda")
    wide[:, 7:7 + n] = dev(v)
    fill = np.complex64(complex(np.float32(-7.25), np.float32(3.5)))
    big = torch.full((F + 12,), complex(fill), dtype=torch.complex64, device="cuda")
    d = pkg.Duc(f, I, decimation=D, gains=a, taps=h, start_index=7)
    assert d.rate.numerator == I and d.rate.denominator == D
    x = d.process_bulk(wide[:, 7:7 + n], out=big[3:])
    assert tuple(x.shape) == (F,)
    b = host(big)
    assert np.array_equal(bits(b[3:3 + F]), bits(full))
    assert np.all(b[:3] == fill) and np.all(b[3 + F:] == fill)
    # reset(): the stream from start_index again (the first item makes samples 0 .. 6: 7 D > I)
    d.reset()
    assert d.output_items(0) == 0 and d.output_items(1) == 7 and d.output_items(4) == 25
    assert np.array_equal(bits(host(d.process_bulk(dev(v)))), bits(full))
    assert d.frequencies.tolist() == [dref.quantised(t) for t in f]
    # without taps the pair is reduced, with taps a reducible pair is refused
    r = pkg.Duc(f, 50, decimation=8)
    assert (r.interpolation, r.decimation, r.taps.size) == (25, 4, 300)
    assert np.array_equal(bits(host(r.process_bulk(dev(v)))), bits(run(pkg, v, 25, 4, f, pkg.duc_rational_taps(25, 4))))
    with pytest.raises(pkg.Gr4pmError, match="25 / 4"):
        pkg.Duc(f, 50, decimation=8, taps=h)
    # two handles, each made under a torch stream of its own, interleaved: what each gives alone
    v2 = (rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))).astype(np.complex64)
    f2 = [0.2, -0.44, 0.01]
    full2 = run(pkg, v2, I, D, f2, h)
    va, vb = dev(v), dev(v2)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        c1 = pkg.Duc(f, I, decimation=D, gains=a, taps=h, start_index=7)
    with torch.cuda.stream(s2):
        c2 = pkg.Duc(f2, I, decimation=D, taps=h)
    p1, p2, lo = [], [], 0
    for hi in (200, 201, 900, 1700, n):
        with torch.cuda.stream(s1):
            p1.append(c1.process_bulk(va[:, lo:hi]))
        with torch.cuda.stream(s2):
            p2.append(c2.process_bulk(vb[:, lo:hi]))
        lo = hi
    torch.cuda.synchronize()
    assert np.array_equal(bits(host(torch.cat(p1))), bits(full))
    assert np.array_equal(bits(host(torch.cat(p2))), bits(full2))
    # and interleaved on ONE stream
    c1.reset()
    with torch.cuda.stream(s1):
        c4 = pkg.Duc(f2, I, decimation=D, taps=h)
        p1, p2, lo = [], [], 0
        for hi in (1, 777, n):
            p1.append(c1.process_bulk(va[:, lo:hi]))
            p2.append(c4.process_bulk(vb[:, lo:hi]))
            lo = hi
    torch.cuda.synchronize()
    assert np.array_equal(bits(host(torch.cat(p1))), bits(full))
    assert np.array_equal(bits(host(torch.cat(p2))), bits(full2))


def load_app(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "apps", name + ".py"))
    app = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(app)
    return app


@pytest.mark.timeout(600)
def test_25_over_4_to_packets_end_to_end(pkg, tmp_path):
    """two carriers, each five 64-byte payloads from PacketTransmitter (4 samples per symbol) -> Duc([f0, f1], 25,
    decimation=4) in unequal calls: a wideband stream at 25/4 of the receiver's rate, noiseless, no PfbArbResampler
    anywhere -> Ddc([f0, f1], 25, interpolation=4) in unequal calls -> NativeMultiChannelReceiver(2): as many detector
    tags as bursts per row; every row through NativePacketReceiver: every payload byte for byte.  Then the two file
    apps (their functions, in process): packet_transmitter_file.py --format sc16 --tune 0.13 --interpolate 25/4 writes
    a file and packet_receiver_file.py --format sc16 --tune 0.13 --decimate 25/4 returns its packets."""
    import torch
    carriers = [-0.2, 0.23]
    rng = np.random.default_rng(2028)
    tx = pkg.PacketTransmitter()
    rows, sent = [], []
    for _ in carriers:
        payloads = [rng.integers(0, 256, 64, dtype=np.uint8).tobytes() for _ in range(5)]
        tx.reset()
        b, _, _ = tx.process_bulk(payloads, gaps=[int(g) for g in rng.integers(2500, 4000, 5)])
        rows.append(torch.cat([b, torch.zeros(6000, dtype=torch.complex64, device="cuda")]))
        sent.append(payloads)
    n = max(r.numel() for r in rows)
    v = torch.zeros((2, n), dtype=torch.complex64, device="cuda")
    for k, r in enumerate(rows):
        v[k, :r.numel()] = r
    u = pkg.Duc(carriers, 25, decimation=4, max_items=n)
    assert u.rate * 4 == 25
    parts, lo = [], 0
    for hi in (7001, 7002, 18999, n):
        parts.append(u.process_bulk(v[:, lo:hi]))
        lo = hi
    x = torch.cat(parts).contiguous()
    assert tuple(x.shape) == (rref.sample_count(n, 25, 4),)

    d = pkg.Ddc(carriers, 25, interpolation=4)
    parts, lo = [], 0
    for hi in (25 * 700 + 3, 25 * 700 + 4, 25 * 1900 - 1, x.numel()):
        parts.append(d.process_bulk(x[lo:hi]))
        lo = hi
    y = torch.cat(parts, dim=1).contiguous()
    N = x.numel() * 4 // 25
    assert tuple(y.shape) == (2, N)
    got = pkg.NativeMultiChannelReceiver(2, syncword_threshold=20.0, max_items=N).process_bulk(y)
    for k in range(2):
        tags = got[k]["detector_tags"]["index"]
        print(f"\n[rational duc end to end] row {k}: tags at {tags.tolist()}")
        assert tags.size == len(sent[k]), (k, tags)
    for k in range(2):
        rx = pkg.NativePacketReceiver(max_items=N, tags_cap=2048, syncword_threshold=20.0, decode_headers=True,
                                      packets_only=True)
        assert received_packets(rx.process_bulk(y[k].contiguous())) == sent[k], k

    # the file apps: a gain of 2^12 leaves the components (within +-4) far from clipping
    txa, rxa = load_app("packet_transmitter_file"), load_app("packet_receiver_file")
    assert txa.interpolation("25/4") == (25, 4) and txa.interpolation("5") == (5, 1)
    for bad in ("4/25", "25/0", "x", "25/4/1"):
        with pytest.raises(ValueError):
            txa.interpolation(bad)
    path = str(tmp_path / "wideband.sc16")
    stats = {}
    written = txa.transmit(sent[0], path, gap=3000, pkg=pkg, fmt="sc16", gain=4096.0, stats=stats, tune=0.13,
                           interpolate="25/4")
    assert os.path.getsize(path) == 4 * written and stats["clipped"] == 0
    assert written == rref.sample_count(sum(3000 + 4 * (4 * len(p) + 228) for p in sent[0]) + 13, 25, 4)  # 13: the Duc's tail
    with open(path, "ab") as f:  # silence behind the last burst, as in front of every other one
        f.write(np.zeros((8192 * 25 // 4, 2), dtype=np.int16).tobytes())
    r = rxa.receive_file(path, syncword_threshold=20.0, chunk_items=50000, pkg=pkg, fmt="sc16", scale=1.0 / 4096.0, tune=0.13,
                         decimate="25/4")
    assert r["packets"] == sent[0]


def test_error_paths_return_statuses(pkg):
    import torch
    lib = pkg.lib()
    I, D, K = 25, 4, 3
    f = [0.1, -0.2, 0.3]
    taps = np.full(300, 0.01, np.float32)

    def create(**kw):
        args = dict(f=f, I=I, D=D, gains=None, taps=taps, max_items=100)
        args.update(kw)
        st, h = rational_handle(pkg, args["f"], args["I"], args["D"], args["gains"], args["taps"], 0, args["max_items"])
        if st == 0:
            lib.gr4pm_duc_destroy(h)
        else:
            assert not h.value and lib.gr4pm_last_error()
        return st

    assert create() == 0
    assert create(taps=None) == 0                                    # the default design
    assert create(gains=[1.5, -2.0, 0.25]) == 0
    assert create(I=1023, D=64, taps=np.ones(8192, np.float32)) == 0
    assert create(I=1, D=64, taps=np.ones(8192, np.float32)) == 0
    assert create(I=4, D=2) == -1 and b"2 / 1" in lib.gr4pm_last_error()    # not in lowest terms: the reduced pair
    assert create(I=50, D=8) == -1 and b"25 / 4" in lib.gr4pm_last_error()
    for bad in (dict(D=0), dict(D=65), dict(I=1025), dict(I=0), dict(max_items=0), dict(taps=np.ones(8193, np.float32)),
                dict(f=[]), dict(gains=[1.0, float("nan"), 1.0])):
        assert create(**bad) == -1, bad
    assert create(I=2, D=3, taps=None) == -1 and b"cutoff" in lib.gr4pm_last_error()  # the defaults exist for I >= D only
    assert create(I=2, D=3, taps=np.ones(24, np.float32)) == 0
    assert lib.gr4pm_duc_create_rational(None, None) == -1
    n = C.c_size_t(7)
    assert lib.gr4pm_duc_rational_taps(25, 4, 12, 0.25, 0.75, None) == -1
    with pytest.raises(pkg.Gr4pmError):
        pkg.Duc(f, I, decimation=65)
    with pytest.raises(pkg.Gr4pmError):
        pkg.Duc(f, I, decimation=0)
    with pytest.raises(pkg.Gr4pmError, match="cutoff"):
        pkg.Duc(f, 2, decimation=3)

    d = pkg.Duc(f, I, decimation=D, taps_per_phase=12, max_items=100, start_index=5)
    v = torch.randn((K, 128), dtype=torch.complex64, device="cuda")
    out = torch.zeros(128 * 7, dtype=torch.complex64, device="cuda")
    st = lib.gr4pm_duc_process(d._h, v.data_ptr(), 128, 101, out.data_ptr(), out.numel(), C.byref(n))
    assert st == -5 and n.value == 0 and b"made for" in lib.gr4pm_last_error()          # beyond max_items
    n = C.c_size_t(7)
    st = lib.gr4pm_duc_process(d._h, v.data_ptr(), 128, 50, out.data_ptr(), 312, C.byref(n))  # 313 samples, room for 312
    assert st == -5 and n.value == 0 and b"room" in lib.gr4pm_last_error()
    for args in ((None, 128, 50, out.data_ptr(), out.numel()), (v.data_ptr(), 128, 50, None, out.numel()),
                 (v.data_ptr(), 49, 50, out.data_ptr(), out.numel())):                   # null pointers, in_stride < n_in
        n = C.c_size_t(7)
        assert lib.gr4pm_duc_process(d._h, *args, C.byref(n)) == -1 and n.value == 0 and lib.gr4pm_last_error()
    assert lib.gr4pm_duc_process(d._h, v.data_ptr(), 128, 50, out.data_ptr(), out.numel(), None) == -1
    with pytest.raises(pkg.Gr4pmError):
        d.process_bulk(v[:, :101])
    with pytest.raises(pkg.Gr4pmError):
        d.process_bulk(v[:, :50], out=out[:312])
    with pytest.raises(pkg.Gr4pmError):
        d.process_bulk(v[:2, :50])
    # none of the refused calls moved the stream or wrote anything: the handle still is at its start
    assert d.output_items(1) == 7 and d.output_items(50) == 313 and d.output_items(0) == 0
    assert np.all(host(out) == 0)
    x = d.process_bulk(v[:, :50], out=out)
    assert tuple(x.shape) == (313,)
    fresh = pkg.Duc(f, I, decimation=D, taps_per_phase=12, start_index=5).process_bulk(v[:, :50])
    assert np.array_equal(bits(host(x)), bits(host(fresh)))
    assert np.max(np.abs(host(x))) > 0
    assert d.output_items(1) == 6  # 51 items make 319 samples: the count depends on the position
    assert d.process_bulk(v[:, :0]).shape[0] == 0
