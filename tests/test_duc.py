"""The Duc on the GPU: every output sample against the float64 statement of its definition within a derived bound (also
from start indices beyond 2^32); exact properties (call cuts, power-of-two scaling and gains, the identity, row stride,
reset, two handles); PacketTransmitter -> Duc -> noise -> Ddc -> receivers -> payload bytes; error paths.  The kernel
has one form (instantiated for 1, 2, 4 and 8 phases per lane), so there is no fast-against-generic test.

The bound of the float64 tests, per output sample j = m I + r:
    |x - x64| <= C * 2^-24 * S[j],   S[j] = sum_k |a_k| (sum_p |h[p I + r]|) max_p |v_k[m - p]|,   C = 3 K P + 8
Each component of each complex multiply-accumulate takes two roundings, a component's error reaches the magnitude with
a factor of 2 sqrt(2) < 3, and the sequential sum has K P terms; 8 covers the rounding of the rotated taps, the rotator
and its product.  First order, worst case: not a fit."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _ddc_ref as dref
import _duc_ref as uref
from _frontend import FREQ_POOL, bits, dev, host, load_package, random_taps, received_packets

pytestmark = pytest.mark.gpu

SIZES = [(5, 60, 3), (4, 48, 1), (64, 768, 8), (1, 1, 1), (20, 161, 16), (3, 97, 2), (1000, 2000, 2), (16, 8192, 9),
         (2, 24, 64)]
GAIN_POOL = [1.0, -0.5, 2.0, 0.75, 1.25, -1.0, 3.0, 0.125]


def freqs_of(I, L, K):
    o = SIZES.index((I, L, K)) if (I, L, K) in SIZES else 0
    return [FREQ_POOL[(o + k) % len(FREQ_POOL)] for k in range(K)]


def gains_of(K):
    """None (the C ABI's NULL) for one row, else a pool with signs and values that are no power of two"""
    return None if K == 1 else [GAIN_POOL[k % len(GAIN_POOL)] for k in range(K)]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def default_taps(pkg, I, L):
    """the default design where L is a multiple of I, else the same design at L taps"""
    if L % I == 0:
        return pkg.duc_taps(I, L // I)
    return (I * dref.kaiser_taps64(I, L)).astype(np.float32)


def items_of(I, L):
    """n I <= 2^21 and n >= 40 P where that fits"""
    P = -(-L // I)
    return min((1 << 21) // I, max(40 * P, 3000))


def dynamic_rows(K, n, P, seed=1):
    """noise rows cut into segments scaled 2^-20, 1, 2^10 and 2^-64, a stretch of exact zeros in each of the first
    three, and unit impulses at the first, the second and the last item with silence between them and the noise"""
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))).astype(np.complex64)
    q = n // 4
    for s, e in enumerate((-20, 0, 10, -64)):
        v[:, s * q:(n if s == 3 else (s + 1) * q)] *= np.float32(2.0 ** e)
    gap = max(2, min(2 * P + 2, n // 16))
    for s in range(1, 3):
        v[:, s * q + q // 2:s * q + q // 2 + gap] = 0
    v[:, :2 * gap] = 0
    v[:, n - 2 * gap:] = 0
    v[:, 0] = 1.0
    v[:, 1] = 1.0j
    v[:, n - 1] = 1.0
    return v


def run(pkg, v, I, freqs, taps, gains=None, cuts=None, start=0):
    """the rows through one handle in one call, or cut at `cuts` (item positions); [n I] on the host"""
    import torch
    d = pkg.Duc(freqs, I, gains=gains, taps=taps, start_index=start, max_items=max(v.shape[1], 1))
    vd = dev(v)
    parts, lo = [], 0
    for hi in list(cuts or []) + [v.shape[1]]:
        want = d.output_items(hi - lo)
        assert want == (hi - lo) * I
        parts.append(d.process_bulk(vd[:, lo:hi]))
        assert parts[-1].shape == (want,)
        lo = hi
    return host(torch.cat(parts))


def ratio(x, x64, v, h, I, gains):
    """|x - x64| / (2^-24 S); samples with S = 0 must be exactly zero"""
    S = uref.window_scale(v, h.astype(np.float64), I, gains)
    err = np.abs(x.astype(np.complex128) - x64)
    assert np.all(x[S == 0] == 0)
    nz = S > 0
    return err[nz] / (dref.EPS32 * S[nz])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("I,L,K", SIZES)
def test_against_float64(pkg, I, L, K):
    """every output sample within C = 3 K P + 8 of the float64 rotated-taps form (pinned to the definition by
    tests/test_duc_ref.py), the default design and a random-sign prototype.  Measured on MI355X (max / rms of the
    ratio): see DESIGN.md section 17"""
    P = -(-L // I)
    n = items_of(I, L)
    v = dynamic_rows(K, n, P)
    f, a = freqs_of(I, L, K), gains_of(K)
    Cb = 3 * K * P + 8
    for name, h in (("default", default_taps(pkg, I, L)), ("random", random_taps(I, L, 3))):
        x64 = uref.duc64_rotated(v, h.astype(np.float64), I, f, a)
        x = run(pkg, v, I, f, h, a)
        assert x.shape == x64.shape == (n * I,)
        r = ratio(x, x64, v, h, I, a)
        print(f"\n[duc float64] I = {I}, L = {L}, K = {K}, {name} taps: max ratio {r.max():.3f}, "
              f"rms {np.sqrt(np.mean(r ** 2)):.4f} (C = {Cb})")
        assert r.max() <= Cb
        assert np.max(np.abs(x64)) > 50.0  # the stimulus: the 2^10 segment reaches the output


@pytest.mark.timeout(300)
@pytest.mark.parametrize("start", [(1 << 32) - 1000, (1 << 40) + 3])
def test_start_index(pkg, start):
    """a phase computed in float, or one that overflows, does not survive a stream that starts here (the first start
    crosses 2^32 at output sample 1000, inside frame 200)"""
    I, L, K = 5, 60, 3
    P = L // I
    rng = np.random.default_rng(17)
    n = 4000
    v = (rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))).astype(np.complex64)
    f = [-0.3137, 3.0 * 2.0 ** -32, 0.123456789]
    a = gains_of(K)
    h = random_taps(I, L, 4)
    x64 = uref.duc64_rotated(v, h.astype(np.float64), I, f, a, start)
    samples = [0, 1, 5, 997, 998, 999, 1000, 1001, 1002, 1004, 1005, n * I - 1]
    direct = uref.duc64_direct(v, h.astype(np.float64), I, f, a, start, samples)
    S = uref.window_scale(v, h.astype(np.float64), I, a)
    assert np.all(np.abs(x64[samples] - direct) <= 1e-12 * S[samples])
    x = run(pkg, v, I, f, h, a, cuts=[155, 1401], start=start)
    Cb = 3 * K * P + 8
    r = ratio(x, x64, v, h, I, a)
    print(f"\n[duc start_index] start = {start}: max ratio {r.max():.3f}, rms {np.sqrt(np.mean(r ** 2)):.4f} (C = {Cb})")
    assert r.max() <= Cb
    assert np.all(np.abs(x[samples] - direct) <= Cb * dref.EPS32 * S[samples])
    # and the start is not ignored
    assert np.max(np.abs(x - uref.duc64_rotated(v, h.astype(np.float64), I, f, a, 0))) > 0.1


@pytest.mark.timeout(300)
@pytest.mark.parametrize("I,L,K", [(5, 60, 3), (64, 768, 8), (1000, 2000, 2), (1, 1, 1)])
def test_one_call_equals_any_chain_of_calls(pkg, I, L, K):
    rng = np.random.default_rng(I + L)
    P = -(-L // I)
    n = 1500 if I <= 64 else 200
    v = (rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))).astype(np.complex64)
    h = random_taps(I, L, 1)
    f, a = freqs_of(I, L, K), gains_of(K)
    one = run(pkg, v, I, f, h, a, start=12345)
    assert one.shape == (n * I,)
    steps = [0, 1, 1, 1, 2, P - 1, P, P + 1, 0, 0, 1, 3]
    cuts, pos = [], 0
    for s in steps + [int(t) for t in rng.integers(0, 4, 30)] + [int(t) for t in rng.integers(0, 9 * P + 40, 8)]:
        if pos + s <= n:
            pos += s
            cuts.append(pos)
    assert len(cuts) > 30
    assert np.array_equal(bits(run(pkg, v, I, f, h, a, cuts, start=12345)), bits(one))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("I,L,K", [(5, 60, 3), (16, 192, 8)])
def test_power_of_two_scaling_is_exact(pkg, I, L, K):
    """rows times 2^7 and 2^-9: the output times the same, bit for bit (no denormals anywhere: the rows' components are
    normal or exactly zero and far from the ends of the range); gains of 2^e: the bits of scaling row k by 2^e"""
    rng = np.random.default_rng(5)
    n = 1200
    P = L // I
    v = (rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))).astype(np.complex64)
    v[:, 300:300 + 2 * P] = 0
    h = default_taps(pkg, I, L)
    f = freqs_of(I, L, K)
    x0 = run(pkg, v, I, f, h)
    assert np.max(np.abs(x0)) > 1.0
    for k in (7, -9):
        s = np.float32(2.0 ** k)
        vs = (v * s).astype(np.complex64)
        assert np.array_equal(vs / s, v)
        assert np.array_equal(bits(run(pkg, vs, I, f, h)), bits((x0 * s).astype(np.complex64))), k
    e = [(-1.0) ** k * 2.0 ** ((3 * k) % 7 - 3) for k in range(K)]
    ve = (v * np.asarray(e, np.float32)[:, None]).astype(np.complex64)
    assert np.array_equal(bits(run(pkg, v, I, f, h, gains=e)), bits(run(pkg, ve, I, f, h)))


@pytest.mark.timeout(300)
def test_identity(pkg):
    rng = np.random.default_rng(21)
    v = (rng.standard_normal(5001) + 1j * rng.standard_normal(5001)).astype(np.complex64)
    one = np.ones(1, np.float32)
    x = run(pkg, v[None, :], 1, [0.0], one, cuts=[1, 1000])
    assert x.shape == v.shape and np.all(x == v)
    # f = 0.25: the rotator is j^i exactly, and so is its product
    for start in (0, 3, (1 << 32) - 2):
        x = run(pkg, v[None, :], 1, [0.25], one, cuts=[2], start=start)
        want = v.astype(np.complex128) * np.array([1, 1j, -1, -1j])[(np.arange(v.size) + start) % 4]
        assert np.all(x == want.astype(np.complex64))
    # a 1-D tensor is the one row of a one-channel handle
    d = pkg.Duc([0.0], 1, taps=one)
    assert np.all(host(d.process_bulk(dev(v))) == v)


@pytest.mark.timeout(300)
def test_stride_reset_two_handles(pkg):
    import torch
    I, L, K = 5, 60, 3
    rng = np.random.default_rng(9)
    n = 5003
    v = (rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))).astype(np.complex64)
    h = default_taps(pkg, I, L)
    f, a = freqs_of(I, L, K), gains_of(K)
    full = run(pkg, v, I, f, h, a, start=7)
    # rows as a window of a wider tensor, at an odd item offset; the result into a caller's tensor at an odd offset
    # (8-byte aligned only), room to spare untouched
    wide = torch.full((K, n + 45), 3.0 - 2.0j, dtype=torch.complex64, device="cuda")
    wide[:, 7:7 + n] = dev(v)
    fill = np.complex64(complex(np.float32(-7.25), np.float32(3.5)))
    big = torch.full((n * I + 12,), complex(fill), dtype=torch.complex64, device="cuda")
    d = pkg.Duc(f, I, gains=a, taps=h, start_index=7)
    x = d.process_bulk(wide[:, 7:7 + n], out=big[3:])
    assert tuple(x.shape) == (n * I,)
    b = host(big)
    assert np.array_equal(bits(b[3:3 + n * I]), bits(full))
    assert np.all(b[:3] == fill) and np.all(b[3 + n * I:] == fill)
    # reset(): the stream from start_index again
    d.reset()
    assert np.array_equal(bits(host(d.process_bulk(dev(v)))), bits(full))
    # frequencies: w / 2^32 folded to [-0.5, 0.5)
    assert d.frequencies.dtype == np.float64
    assert d.frequencies.tolist() == [dref.quantised(t) for t in f]
    q = pkg.Duc([0.5, -0.25, 3.0 * 2.0 ** -32, 1.75, 0.1], I).frequencies.tolist()
    assert q == [-0.5, -0.25, 3.0 * 2.0 ** -32, -0.25, dref.frequency_word(0.1) / 2.0 ** 32]
    # two handles, each made under a torch stream of its own, interleaved: what each gives alone
    v2 = (rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))).astype(np.complex64)
    f2 = [0.2, -0.44, 0.01]
    full2 = run(pkg, v2, I, f2, h)
    va, vb = dev(v), dev(v2)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        c1 = pkg.Duc(f, I, gains=a, taps=h, start_index=7)
    with torch.cuda.stream(s2):
        c2 = pkg.Duc(f2, I, taps=h)
    p1, p2, lo = [], [], 0
    for hi in (200, 201, 1800, 4000, n):
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
    c3 = pkg.Duc(f2, I, taps=h)
    with torch.cuda.stream(s1):
        c4 = pkg.Duc(f2, I, taps=h)
        p1, p2, lo = [], [], 0
        for hi in (1, 777, n):
            p1.append(c1.process_bulk(va[:, lo:hi]))
            p2.append(c4.process_bulk(vb[:, lo:hi]))
            lo = hi
    torch.cuda.synchronize()
    assert np.array_equal(bits(host(torch.cat(p1))), bits(full))
    assert np.array_equal(bits(host(torch.cat(p2))), bits(full2))
    assert np.array_equal(bits(host(c3.process_bulk(vb))), bits(full2))


@pytest.mark.timeout(600)
def test_duc_to_packets_end_to_end(pkg):
    """I = D = 5, four carriers at -0.37, -0.11, +0.13, +0.41 cycles per sample, each with three bursts of distinct
    random payloads from PacketTransmitter and a CFO of its own; Duc (four unequal calls) -> NoiseSource of sigma 0.05
    added on the wideband stream -> Ddc (four unequal calls) -> NativeMultiChannelReceiver: per row as many detector
    tags as bursts; every row through NativePacketReceiver: every payload byte for byte.  The Duc's output is within
    the float64 bound of duc64_rotated on the same rows.  syncword_threshold is 20.0 as in tests/test_ddc.py.  The
    noise seed is 5, the first one tried."""
    import torch
    I, P, N = 5, 12, 30000
    carriers = [-0.37, -0.11, 0.13, 0.41]
    K = len(carriers)
    rng = np.random.default_rng(2026)
    tx = pkg.PacketTransmitter()
    v = torch.zeros((K, N), dtype=torch.complex64, device="cuda")
    sent = []
    for k in range(K):
        payloads = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(30, 200, 3)]
        gaps = [int(g) for g in rng.integers(2500, 4000, 3)]
        tx.reset()
        b, _, _ = tx.process_bulk(payloads, gaps=gaps)
        assert b.numel() + 9000 < N
        cfo = float(rng.uniform(-0.03, 0.03))  # rad / item; the detector's +-4 bins reach +-0.042
        rot = torch.exp(1j * cfo * torch.arange(b.numel(), device="cuda", dtype=torch.float64))
        v[k, :b.numel()] = (b.to(torch.complex128) * rot).to(torch.complex64)
        sent.append(payloads)
    torch.cuda.synchronize()

    hu = pkg.duc_taps(I, P)
    u = pkg.Duc(carriers, I, taps=hu)
    assert u.frequencies.tolist() == [dref.quantised(f) for f in carriers]
    parts, lo = [], 0
    for hi in (7001, 7002, 18999, N):
        parts.append(u.process_bulk(v[:, lo:hi]))
        lo = hi
    x = torch.cat(parts).contiguous()
    assert tuple(x.shape) == (N * I,)
    vh = host(v)
    r = ratio(host(x), uref.duc64_rotated(vh, hu.astype(np.float64), I, carriers), vh, hu, I, None)
    print(f"\n[duc end to end] Duc against float64: max ratio {r.max():.3f} (C = {3 * K * P + 8})")
    assert r.max() <= 3 * K * P + 8

    x = pkg.NoiseSource("gaussian", 0.05, 5, "c64", max_items=N * I).process_bulk(N * I, add_to=x)
    d = pkg.Ddc(carriers, I, taps=pkg.ddc_taps(I, P))
    parts, lo = [], 0
    for hi in (I * 7000 + 3, I * 7000 + 4, I * 19000 - 1, N * I):
        parts.append(d.process_bulk(x[lo:hi]))
        lo = hi
    y = torch.cat(parts, dim=1).contiguous()
    assert tuple(y.shape) == (K, N)

    got = pkg.NativeMultiChannelReceiver(K, syncword_threshold=20.0, max_items=N).process_bulk(y)
    for k in range(K):
        t = got[k]["detector_tags"]["index"].astype(np.int64)
        print(f"\n[duc end to end] row {k}: tags at {t.tolist()}")
        assert t.size == len(sent[k]), (k, t)
    for k in range(K):
        rx = pkg.NativePacketReceiver(max_items=N, tags_cap=2048, syncword_threshold=20.0, decode_headers=True,
                                      packets_only=True)
        assert received_packets(rx.process_bulk(y[k].contiguous())) == sent[k], k


def test_error_paths_return_statuses(pkg):
    import torch
    L = pkg.lib()
    abi = importlib.import_module(pkg.__name__ + "._abi")
    I, K = 5, 3
    fr = (C.c_double * 65)(*([0.1] * 65))
    ga = (C.c_double * 65)(*([1.5] * 65))
    tp = (C.c_float * 8193)(*([0.01] * 8193))

    def create(n_channels=K, interpolation=I, frequencies=fr, gains=ga, taps=tp, n_taps=60, max_items=100, start_index=0):
        p = abi.DucParams(n_channels, interpolation, C.cast(frequencies, C.c_void_p), C.cast(gains, C.c_void_p),
                          C.cast(taps, C.c_void_p), n_taps, max_items, start_index, None)
        h = C.c_void_p(0x1234)
        st = L.gr4pm_duc_create(C.byref(p), C.byref(h))
        if st == 0:
            L.gr4pm_duc_destroy(h)
        else:
            assert not h.value and L.gr4pm_last_error()
        return st

    assert create() == 0
    assert create(taps=None, n_taps=0) == 0  # the default design
    assert create(gains=None) == 0           # all 1
    assert create(n_taps=8192, interpolation=1024) == 0
    assert create(n_taps=8192, interpolation=1) == 0
    assert create(n_channels=64) == 0
    for bad in (dict(n_channels=0), dict(n_channels=65), dict(interpolation=0), dict(interpolation=1025), dict(n_taps=0),
                dict(n_taps=8193), dict(frequencies=None), dict(max_items=0)):
        assert create(**bad) == -1, bad
    for t in (float("nan"), float("inf"), -float("inf")):
        bad_f = (C.c_double * 3)(0.1, 0.2, t)
        assert create(frequencies=bad_f) == -1 and b"frequencies[2] is not finite" in L.gr4pm_last_error()
        assert create(gains=bad_f) == -1 and b"gains[2] is not finite" in L.gr4pm_last_error()
    assert L.gr4pm_duc_create(None, None) == -1
    with pytest.raises(pkg.Gr4pmError):
        pkg.Duc([0.1], 5, taps=[])
    with pytest.raises(pkg.Gr4pmError):
        pkg.Duc([], 5)
    with pytest.raises(pkg.Gr4pmError):
        pkg.Duc([0.1, float("nan")], 5)
    with pytest.raises(pkg.Gr4pmError):
        pkg.Duc([0.1, 0.2], 5, gains=[1.0])
    with pytest.raises(pkg.Gr4pmError):
        pkg.Duc([0.1, 0.2], 5, gains=[1.0, float("inf")])

    d = pkg.Duc([0.1, -0.2, 0.3], I, taps_per_phase=12, max_items=100, start_index=5)
    v = torch.randn((K, 128), dtype=torch.complex64, device="cuda")
    out = torch.zeros(128 * I, dtype=torch.complex64, device="cuda")
    n = C.c_size_t(7)
    st = L.gr4pm_duc_process(d._h, v.data_ptr(), 128, 101, out.data_ptr(), 128 * I, C.byref(n))
    assert st == -5 and n.value == 0 and b"made for" in L.gr4pm_last_error()          # beyond max_items
    n = C.c_size_t(7)
    st = L.gr4pm_duc_process(d._h, v.data_ptr(), 128, 50, out.data_ptr(), 50 * I - 1, C.byref(n))
    assert st == -5 and n.value == 0 and b"room" in L.gr4pm_last_error()              # out_cap too small
    for args in ((None, 128, 50, out.data_ptr(), 128 * I), (v.data_ptr(), 128, 50, None, 128 * I),
                 (v.data_ptr(), 49, 50, out.data_ptr(), 128 * I)):                     # null pointers, in_stride < n_in
        n = C.c_size_t(7)
        assert L.gr4pm_duc_process(d._h, *args, C.byref(n)) == -1 and n.value == 0 and L.gr4pm_last_error()
    assert L.gr4pm_duc_process(d._h, v.data_ptr(), 128, 50, out.data_ptr(), 128 * I, None) == -1
    assert L.gr4pm_duc_process(None, v.data_ptr(), 128, 50, out.data_ptr(), 128 * I, C.byref(n)) == -1
    assert L.gr4pm_duc_frequencies(d._h, None) == -1 and L.gr4pm_duc_output_items(d._h, 5, None) == -1
    assert L.gr4pm_duc_reset(None) == -1
    with pytest.raises(pkg.Gr4pmError):
        d.process_bulk(v[:, :101])
    with pytest.raises(pkg.Gr4pmError):
        d.process_bulk(v[:, :50], out=out[:50 * I - 1])
    with pytest.raises(pkg.Gr4pmError):
        d.process_bulk(v[:2, :50])
    # none of the refused calls moved the stream or wrote anything: the handle still is at its start
    assert np.all(host(out) == 0)
    x = d.process_bulk(v[:, :50], out=out)
    assert tuple(x.shape) == (50 * I,)
    fresh = pkg.Duc([0.1, -0.2, 0.3], I, taps_per_phase=12, start_index=5).process_bulk(v[:, :50])
    assert np.array_equal(bits(host(x)), bits(host(fresh)))
    assert d.process_bulk(v[:, :0]).shape[0] == 0
