"""The Ddc resampling by I / D on the GPU (gr4pm_ddc_create_rational): every output item
against the float64 statement of its definition within a derived bound (also from start indices beyond 2^32); exact
properties (every branch is an integer Ddc bit for bit, I = 1 is the integer Ddc, call cuts, integer ingest, row
stride, reset, two handles); wideband IQ at 25/4 of the receiver's rate -> Ddc -> receiver -> payload bytes, and the
file app on the same stream; error paths.

The bound of the float64 tests, per output item n of branch p_n:
    |y - y64| <= C * 2^-24 * sum_s |h[p_n + s I]| * max |x| over the item's P samples,   C = P + 8,  P = ceil(L / I)
P for the sum accumulated in sequence, 8 for the rounding of the rotated taps, the complex products and the rotator
with its product (section 16's derivation with the branch's P taps).  First order, worst case: not a fit.

Shapes (I, D, L, K).  The list asked for names (2, 1000, 2000, 2) as "a tile of few frames", but 2 / 1000 is not in
lowest terms and the definition refuses such a pair (the refusal is tested below); (2, 1001, 2000, 2) stands in: the
same I, L and K and a larger D, so a tile of no more frames.  The default design's band edges are in units of the
output rate and refused beyond half of the input rate, so the shapes with I > D take the design at edges scaled by
D / I."""
import ctypes as C
import importlib
import importlib.util
import os

import numpy as np
import pytest

import _ddc_rational_ref as rref
from _frontend import (FREQ_POOL, bits, dev, exact_iq_forms, host, load_package, random_taps, received_packets,
                       short_calls_of_mixed_formats)
from test_ddc import dynamic_stream

pytestmark = pytest.mark.gpu

SIZES = [(4, 25, 300, 3), (3, 2, 24, 1), (5, 12, 61, 2), (7, 1, 30, 1), (2, 1001, 2000, 2), (63, 64, 768, 16),
         (64, 1023, 8192, 9), (8, 3, 5, 2)]  # the last one: L < I, branches 5 .. 7 have no tap and give exact zeros


def freqs_of(I, D, L, K):
    o = SIZES.index((I, D, L, K)) if (I, D, L, K) in SIZES else 0
    return [FREQ_POOL[(o + k) % len(FREQ_POOL)] for k in range(K)]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def default_taps(pkg, I, D, L):
    """the default design (band edges scaled by D / I where I > D) where L is a multiple of D, else the same design at
    L taps"""
    m = min(1.0, D / I)
    if L % D == 0:
        return pkg.ddc_rational_taps(I, D, L // D, 0.25 * m, 0.75 * m)
    return rref.rational_taps64(I, D, L, 0.25 * m, 0.75 * m).astype(np.float32)


def run(pkg, x, I, D, freqs, taps, cuts=None, start=0):
    """the stream through one handle in one call, or cut at `cuts`; [K, items] on the host.  output_items is exact
    before each call"""
    import torch
    d = pkg.Ddc(freqs, D, interpolation=I, taps=taps, start_index=start, max_frames=x.size * I // D + I + 1)
    assert (d.interpolation, d.decimation) == (I, D)
    xd = dev(x)
    parts, lo = [], 0
    for hi in list(cuts or []) + [x.size]:
        want = d.output_items(hi - lo)
        assert want == hi * I // D - lo * I // D
        parts.append(d.process_bulk(xd[lo:hi]))
        assert parts[-1].shape[1] == want
        lo = hi
    return host(torch.cat(parts, dim=1))


def ratio(y, y64, x, h, I, D):
    """|y - y64| / (2^-24 sum_s |h[p_n + s I]| max|x| over the window); items whose window is all zeros must be
    exactly zero"""
    j, p = rref.items(x.size, I, D)
    wm = rref.window_max(x, j, -(-h.size // I))
    scale = rref.EPS32 * rref.branch_abs_sum(h.astype(np.float64), I)[p] * wm
    err = np.abs(y.astype(np.complex128) - y64)
    assert np.all(y[:, scale == 0] == 0)  # a window of zeros, or a branch without taps (L < I)
    nz = scale > 0
    return err[:, nz] / scale[nz][None, :]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("I,D,L,K", SIZES)
def test_against_float64(pkg, I, D, L, K):
    """every output item within C = P + 8 of the float64 rotated-taps form (pinned to the definition by
    tests/test_ddc_rational_ref.py), the default design and a random prototype.  Max / rms of the ratio as measured on MI355X: DESIGN.md
    section 18's accuracy table (the largest is 6.437 at (63, 64, 768, 16), C = 21)"""
    x = dynamic_stream(D)
    f = freqs_of(I, D, L, K)
    P = -(-L // I)
    Cb = P + 8
    for name, h in (("default", default_taps(pkg, I, D, L)), ("random", random_taps(D, L, 3))):
        y64 = rref.rddc64_rotated(x, h.astype(np.float64), I, D, f)
        y = run(pkg, x, I, D, f, h)
        assert y.shape == y64.shape == (K, x.size * I // D)
        r = ratio(y, y64, x, h, I, D)
        print(f"\n[rational ddc float64] I = {I}, D = {D}, L = {L}, K = {K}, {name} taps: max ratio {r.max():.3f}, "
              f"rms {np.sqrt(np.mean(r ** 2)):.4f} (C = {Cb})")
        assert r.max() <= Cb
        if name == "random":  # the stimulus: the 2^10 segment reaches the output
            assert np.max(np.abs(y64)) > 50.0
        if L < I:
            assert np.any(rref.branch_abs_sum(h.astype(np.float64), I) == 0) and np.max(np.abs(y)) > 0


@pytest.mark.timeout(300)
@pytest.mark.parametrize("I,D,L,K", [(4, 25, 300, 3), (5, 12, 61, 2)])
def test_every_branch_is_an_integer_ddc_bit_for_bit(pkg, I, D, L, K):
    """the items n_p + I j of branch p against Ddc(f, D, taps=h[p::I], start_index=S - z) on zeros(z) ++ x: the same
    samples, taps, order and rotator, so the same bits (np.array_equal: -0 equals +0)"""
    rng = np.random.default_rng(I * D)
    n = 150 * D + 7
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    h = random_taps(D, L, 5)
    f = freqs_of(I, D, L, K)
    S = 3 * D + 1
    y = run(pkg, x, I, D, f, h, start=S)
    j, p = rref.items(n, I, D)
    for b in range(I):
        idx = np.nonzero(p == b)[0]
        z = (D - 1 - int(j[idx[0]])) % D
        d = pkg.Ddc(f, D, taps=h[b::I], start_index=S - z)
        yi = host(d.process_bulk(dev(np.concatenate([np.zeros(z, np.complex64), x]))))
        n_int = (j[idx] + z - D + 1) // D
        assert np.all((j[idx] + z - D + 1) % D == 0) and n_int[0] >= 0 and n_int[-1] < yi.shape[1]
        assert np.array_equal(y[:, idx], yi[:, n_int]), b
        assert np.max(np.abs(y[:, idx])) > 0


def rational_handle(pkg, f, I, D, taps=None, start=0, max_frames=1 << 20):
    """gr4pm_ddc_create_rational by hand: (status, handle)"""
    abi = importlib.import_module(pkg.__name__ + "._abi")
    fr = (C.c_double * len(f))(*f)
    tp = None if taps is None else np.ascontiguousarray(taps, np.float32)
    p = abi.DdcRationalParams(len(f), D, C.cast(fr, C.c_void_p), None if tp is None else tp.ctypes.data,
                              0 if tp is None else tp.size, max_frames, start, None, I)
    h = C.c_void_p(0x1234)
    return pkg.lib().gr4pm_ddc_create_rational(C.byref(p), C.byref(h)), h


@pytest.mark.parametrize("D,L,K", [(5, 60, 3), (64, 768, 8)])
def test_interpolation_one_through_create_rational(pkg, D, L, K):
    import torch
    lib = pkg.lib()
    rng = np.random.default_rng(D)
    n = 300 * D + 3
    x = dev((rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64))
    f = [FREQ_POOL[(1 + k) % len(FREQ_POOL)] for k in range(K)]
    st, h = rational_handle(pkg, f, 1, D, start=77)
    assert st == 0 and h.value
    try:
        got_n = C.c_size_t(0)
        assert lib.gr4pm_ddc_output_items(h, n, C.byref(got_n)) == 0 and got_n.value == n // D
        out = torch.zeros((K, n // D), dtype=torch.complex64, device="cuda")
        assert lib.gr4pm_ddc_process(h, x.data_ptr(), n, out.data_ptr(), n // D, n // D, C.byref(got_n)) == 0
        assert got_n.value == n // D
        want = pkg.Ddc(f, D, start_index=77)
        assert want.taps.size == L
        assert np.array_equal(bits(host(out)), bits(host(want.process_bulk(x))))
        assert np.max(np.abs(host(out))) > 0
    finally:
        lib.gr4pm_ddc_destroy(h)


def random_cuts(rng, n, I, D, L):
    """runs of 1-sample calls, empty calls, calls that make no item (D > I) or several per sample (I > D), random ones"""
    P = -(-L // I)
    steps = [0, 1, 1, 1, 1, 1, 1, 1, 0, 0, 2, D - 1, D, D + 1, P - 1, P, 1, 1, 1, 2 * D - 1, 3]
    steps += [int(v) for v in rng.integers(0, 3 * D + 1, 40)] + [int(v) for v in rng.integers(0, 9 * max(P, D), 6)]
    cuts, pos = [], 0
    for s in steps:
        if pos + s <= n:
            pos += s
            cuts.append(pos)
    return cuts


@pytest.mark.timeout(300)
@pytest.mark.parametrize("I,D,L,K", [(4, 25, 300, 3), (3, 2, 24, 1), (64, 1023, 8192, 9)])
def test_one_call_equals_any_chain_of_calls(pkg, I, D, L, K):
    rng = np.random.default_rng(I + D + L)
    n = 300 * D + D // 2 + 3 if D <= 64 else 40 * D + 5
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    h = random_taps(D, L, 1)
    f = freqs_of(I, D, L, K)
    one = run(pkg, x, I, D, f, h, start=12345)
    assert one.shape == (K, n * I // D)
    cuts = random_cuts(rng, n, I, D, L)
    assert len(cuts) > 30
    per_call = np.diff([0] + cuts)
    made = np.diff([0] + [c * I // D for c in cuts])
    assert np.any((per_call > 0) & (made == 0)) or I > D
    assert I <= D or np.any(made > per_call)
    assert np.array_equal(bits(run(pkg, x, I, D, f, h, cuts, start=12345)), bits(one))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("start", [(1 << 32) - 1000, (1 << 40) + 3])
def test_start_index(pkg, start):
    I, D, L, K = 4, 25, 300, 3
    P = -(-L // I)
    rng = np.random.default_rng(17)
    n = 900 * D + 3
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    f = [-0.3137, 3.0 * 2.0 ** -32, 0.123456789]
    h = random_taps(D, L, 4)
    y64 = rref.rddc64_rotated(x, h.astype(np.float64), I, D, f, start)
    which = [0, 1, 159, 160, 161, n * I // D - 1]  # sample 1000 is item 160's
    direct = rref.rddc64_direct(x, h.astype(np.float64), I, D, f, start, which)
    assert np.max(np.abs(y64[:, which] - direct)) <= 1e-12 * np.sum(np.abs(h)) * np.max(np.abs(x))
    y = run(pkg, x, I, D, f, h, cuts=[777, 2 * D * 200 + 1], start=start)
    r = ratio(y, y64, x, h, I, D)
    print(f"\n[rational ddc start_index] start = {start}: max ratio {r.max():.3f}, rms {np.sqrt(np.mean(r ** 2)):.4f} "
          f"(C = {P + 8})")
    assert r.max() <= P + 8
    assert np.max(np.abs(y - rref.rddc64_rotated(x, h.astype(np.float64), I, D, f, 0))) > 0.1


def test_start_index_that_moves_no_phase_is_bit_equal(pkg):
    """frequency words that are multiples of 2^20 and a start of 2^40 + 4096: every w (start mod 2^32) is a multiple
    of 2^32, so the handle gives what one started at 0 gives, bit for bit"""
    I, D, L = 4, 25, 300
    rng = np.random.default_rng(18)
    n = 200 * D + 3
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    f = [3 * 2.0 ** -12, -1000 * 2.0 ** -12, 2047 * 2.0 ** -12]
    assert all(rref.frequency_word(v) % (1 << 20) == 0 and rref.frequency_word(v) for v in f)
    h = random_taps(D, L, 4)
    a = run(pkg, x, I, D, f, h, start=0)
    b = run(pkg, x, I, D, f, h, cuts=[1234], start=(1 << 40) + 4096)
    assert np.array_equal(bits(a), bits(b)) and np.max(np.abs(a)) > 0
    assert not np.array_equal(bits(a), bits(run(pkg, x, I, D, f, h, start=(1 << 40) + 4097)))


@pytest.mark.timeout(300)
def test_integer_ingest_is_bit_equal(pkg):
    """process_bulk(v) on integer IQ against process_bulk(iq_unpack(v)), and short calls of mixed formats against one
    complex64 call"""
    I, D, L, K = 4, 25, 300, 3
    rng = np.random.default_rng(8)
    f = freqs_of(I, D, L, K)
    h = random_taps(D, L, 6)
    v16 = dev(rng.integers(-32768, 32768, (2003, 2)).astype(np.int16))
    v8 = dev(rng.integers(-128, 128, (1501, 2)).astype(np.int8))
    vu = dev(rng.integers(0, 256, (1777, 2)).astype(np.uint8))
    a = pkg.Ddc(f, D, interpolation=I, taps=h, start_index=99)
    b = pkg.Ddc(f, D, interpolation=I, taps=h, start_index=99)
    for v, scale in [(v16, None), (vu, None), (v8, 0.37), (v16, 3.0e-5), (vu[:7], 1.0 / 64), (v8[:4], None), (vu, 0.011)]:
        ya, yb = a.process_bulk(v, scale=scale), b.process_bulk(pkg.iq_unpack(v, scale=scale))
        assert ya.shape == yb.shape and np.array_equal(bits(host(ya)), bits(host(yb)))
    assert a.output_items(0) == 0 and np.max(np.abs(host(ya))) > 0
    x, forms = exact_iq_forms(1249, 31)
    one = run(pkg, x, I, D, f, h, start=99)
    got = short_calls_of_mixed_formats(pkg, pkg.Ddc(f, D, interpolation=I, taps=h, start_index=99), x, forms)
    assert one.shape == got.shape == (K, x.size * I // D)
    assert np.array_equal(bits(got), bits(one))
    assert np.all(np.max(np.abs(one), axis=1) > 0)


@pytest.mark.timeout(300)
def test_stride_reset_two_handles(pkg):
    import torch
    I, D, L, K = 4, 25, 300, 3
    rng = np.random.default_rng(9)
    n = 1000 * D + 3
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    h = default_taps(pkg, I, D, L)
    f = freqs_of(I, D, L, K)
    full = run(pkg, x, I, D, f, h, start=7)
    F = n * I // D
    fill = np.complex64(complex(np.float32(-7.25), np.float32(3.5)))
    big = torch.full((K, F + 45), complex(fill), dtype=torch.complex64, device="cuda")
    d = pkg.Ddc(f, D, interpolation=I, taps=h, start_index=7)
    assert d.rate.numerator == I and d.rate.denominator == D
    y = d.process_bulk(dev(x), out=big[:, 5:5 + F + 3])
    assert tuple(y.shape) == (K, F)
    b = host(big)
    assert np.array_equal(bits(b[:, 5:5 + F]), bits(full))
    assert np.all(b[:, :5] == fill) and np.all(b[:, 5 + F:] == fill)
    # reset(): the stream from start_index again (the first item is sample 6's: m = 24)
    d.reset()
    assert d.output_items(6) == 0 and d.output_items(7) == 1 and d.output_items(25) == 4
    assert np.array_equal(bits(host(d.process_bulk(dev(x)))), bits(full))
    assert d.frequencies.tolist() == [rref.dref.quantised(v) for v in f]
    # without taps the pair is reduced, with taps a reducible pair is refused
    r = pkg.Ddc(f, 50, interpolation=8)
    assert (r.interpolation, r.decimation, r.taps.size) == (4, 25, 300)
    assert np.array_equal(bits(host(r.process_bulk(dev(x)))), bits(run(pkg, x, 4, 25, f, pkg.ddc_rational_taps(4, 25))))
    with pytest.raises(pkg.Gr4pmError, match="4 / 25"):
        pkg.Ddc(f, 50, interpolation=8, taps=h)
    # two handles on two streams at once: what each gives alone
    x2 = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    f2 = [0.2, -0.44, 0.01]
    full2 = run(pkg, x2, I, D, f2, h)
    xa, xb = dev(x), dev(x2)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        c1 = pkg.Ddc(f, D, interpolation=I, taps=h, start_index=7)
    with torch.cuda.stream(s2):
        c2 = pkg.Ddc(f2, D, interpolation=I, taps=h)
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
def test_wideband_at_25_over_4_to_packets_end_to_end(pkg, tmp_path):
    """two carriers, each five 64-byte payloads from PacketTransmitter (4 samples per symbol) -> PfbArbResampler(1.25)
    -> Duc([f0, f1], 5): a wideband stream at 25/4 of the receiver's rate, noiseless.  Ddc([f0, f1], 25,
    interpolation=4) in unequal calls -> NativeMultiChannelReceiver(2): as many detector tags as bursts per row; every
    row through NativePacketReceiver: every payload byte for byte.  The same stream as sc16 through
    apps/packet_receiver_file.py --tune f0 --decimate 25/4 (its function, in process): row 0's packets."""
    import torch
    carriers = [-0.2, 0.23]
    rng = np.random.default_rng(2027)
    tx = pkg.PacketTransmitter()
    rows, sent = [], []
    for _ in carriers:
        payloads = [rng.integers(0, 256, 64, dtype=np.uint8).tobytes() for _ in range(5)]
        tx.reset()
        v, _, _ = tx.process_bulk(payloads, gaps=[int(g) for g in rng.integers(2500, 4000, 5)])
        v = torch.cat([v, torch.zeros(6000, dtype=torch.complex64, device="cuda")])
        u, consumed = pkg.PfbArbResampler(rate=1.25).process_bulk(v)
        assert consumed == v.numel() and abs(u.numel() - 1.25 * v.numel()) <= 64
        rows.append(u)
        sent.append(payloads)
    n = max(r.numel() for r in rows)
    v5 = torch.zeros((2, n), dtype=torch.complex64, device="cuda")
    for k, r in enumerate(rows):
        v5[k, :r.numel()] = r
    x = pkg.Duc(carriers, 5, max_items=n).process_bulk(v5).contiguous()
    assert tuple(x.shape) == (5 * n,)

    d = pkg.Ddc(carriers, 25, interpolation=4)
    assert d.rate * 25 == 4
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
        print(f"\n[rational ddc end to end] row {k}: tags at {tags.tolist()}")
        assert tags.size == len(sent[k]), (k, tags)
    for k in range(2):
        rx = pkg.NativePacketReceiver(max_items=N, tags_cap=2048, syncword_threshold=20.0, decode_headers=True,
                                      packets_only=True)
        assert received_packets(rx.process_bulk(y[k].contiguous())) == sent[k], k

    # the file app on the same stream as sc16 (components within +-4: a gain of 2^12)
    assert float(torch.max(torch.abs(torch.view_as_real(x)))) < 7.9
    path = tmp_path / "wideband.sc16"
    host(pkg.iq_pack(x, "sc16", 4096.0)).tofile(str(path))
    spec = importlib.util.spec_from_file_location(
        "packet_receiver_file", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "apps",
                                             "packet_receiver_file.py"))
    app = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(app)
    assert app.decimation("25/4") == (25, 4) and app.decimation("5") == (5, 1)
    r = app.receive_file(str(path), syncword_threshold=20.0, chunk_items=50000, pkg=pkg, fmt="sc16", scale=1.0 / 4096.0,
                         tune=carriers[0], decimate="25/4")
    assert r["packets"] == sent[0]


def test_error_paths_return_statuses(pkg):
    import torch
    lib = pkg.lib()
    I, D, K = 4, 25, 3
    f = [0.1, -0.2, 0.3]
    taps = np.full(300, 0.01, np.float32)

    def create(**kw):
        args = dict(f=f, I=I, D=D, taps=taps, max_frames=100)
        args.update(kw)
        st, h = rational_handle(pkg, args["f"], args["I"], args["D"], args["taps"], 0, args["max_frames"])
        if st == 0:
            lib.gr4pm_ddc_destroy(h)
        else:
            assert not h.value and lib.gr4pm_last_error()
        return st

    assert create() == 0
    assert create(taps=None) == 0                                    # the default design
    assert create(I=64, D=1023, taps=np.ones(8192, np.float32)) == 0
    assert create(I=8, D=50) == -1 and b"4 / 25" in lib.gr4pm_last_error()  # not in lowest terms: the reduced pair
    assert create(I=2, D=1000) == -1 and b"1 / 500" in lib.gr4pm_last_error()
    for bad in (dict(I=0), dict(I=65), dict(D=0), dict(D=1025, I=4), dict(max_frames=0), dict(taps=np.ones(8193, np.float32))):
        assert create(**bad) == -1, bad
    assert create(I=3, D=2, taps=None) == -1 and b"cutoff" in lib.gr4pm_last_error()  # the defaults, beyond fs / 2
    assert lib.gr4pm_ddc_create_rational(None, None) == -1
    with pytest.raises(pkg.Gr4pmError):
        pkg.Ddc(f, D, interpolation=65)
    with pytest.raises(pkg.Gr4pmError):
        pkg.Ddc(f, D, interpolation=0)

    d = pkg.Ddc(f, D, interpolation=I, taps_per_phase=12, max_frames=100, start_index=5)
    x = torch.randn(700, dtype=torch.complex64, device="cuda")
    out = torch.zeros((K, 128), dtype=torch.complex64, device="cuda")
    n = C.c_size_t(7)
    st = lib.gr4pm_ddc_process(d._h, x.data_ptr(), 626, out.data_ptr(), 128, 128, C.byref(n))   # 626 * 4 > 100 * 25
    assert st == -5 and n.value == 0 and b"made for" in lib.gr4pm_last_error()
    n = C.c_size_t(7)
    st = lib.gr4pm_ddc_process(d._h, x.data_ptr(), 500, out.data_ptr(), 128, 79, C.byref(n))    # 80 items, room for 79
    assert st == -5 and n.value == 0
    for args in ((None, 500, out.data_ptr(), 128, 128), (x.data_ptr(), 500, None, 128, 128),
                 (x.data_ptr(), 500, out.data_ptr(), 79, 128)):          # null pointers, out_stride < items with K > 1
        n = C.c_size_t(7)
        assert lib.gr4pm_ddc_process(d._h, *args, C.byref(n)) == -1 and n.value == 0
    assert lib.gr4pm_ddc_process(d._h, x.data_ptr(), 500, out.data_ptr(), 128, 128, None) == -1
    n = C.c_size_t(7)
    assert lib.gr4pm_ddc_process_iq(d._h, x.data_ptr(), 9, 0.0, 500, out.data_ptr(), 128, 128, C.byref(n)) == -1
    assert n.value == 0 and b"format" in lib.gr4pm_last_error()
    with pytest.raises(pkg.Gr4pmError):
        d.process_bulk(x[:626])
    with pytest.raises(pkg.Gr4pmError):
        d.process_bulk(x[:500], out=out[:, :79])
    # none of the refused calls moved the stream or wrote anything
    assert d.output_items(6) == 0 and d.output_items(7) == 1 and d.output_items(625) == 100
    assert np.all(host(out) == 0)
    y = d.process_bulk(x[:500], out=out)
    assert tuple(y.shape) == (K, 80)
    fresh = pkg.Ddc(f, D, interpolation=I, taps_per_phase=12, start_index=5).process_bulk(x[:500])
    assert np.array_equal(bits(host(y)), bits(host(fresh)))
    assert np.max(np.abs(host(y))) > 0
    assert d.process_bulk(x[:0]).shape[1] == 0
