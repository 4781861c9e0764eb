"""The Channelizer on the GPU: every output item against the float64 statement of its definition within a derived
bound; exact properties (call cuts, power-of-two scaling, row subsets, row stride, reset, two handles); the fast and
the generic form bit for bit; wideband IQ -> Channelizer -> NativeMultiChannelReceiver -> payload bytes; error paths.

The bound of the float64 test, per output item:
    |y - y64| <= C * 2^-24 * sum_t |h[t]| * max |x| over the item's L samples,   C = P + 5 log2 M
A P-term branch sum accumulated in sequence is within P u of sum |h| |x| of its branch; each radix-2 level adds at most
about 5 u relative (twiddle rounding, the complex product, the add) to a quantity bounded by the sum of the branch
magnitudes, itself at most sum_t |h[t]| max |x|.  First order, worst case: not a fit."""
import ctypes as C

import numpy as np
import pytest

import _channelizer_ref as cref
import test_syncword_float64 as t64
from _frontend import bits, dev, exact_iq_forms, host, load_package, received_packets, short_calls_of_mixed_formats

pytestmark = pytest.mark.gpu

SIZES = [(16, 12), (64, 12), (256, 8), (2, 1), (1024, 3), (8, 32)]
FAST = [(16, 12), (64, 12), (256, 8), (256, 12)]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def random_taps(M, P, seed=0):
    """a low-pass shape with random signs mixed in: every tap matters, none is tiny"""
    rng = np.random.default_rng(seed)
    h = cref.kaiser_taps64(M, P) * M + 0.05 * rng.standard_normal(P * M)
    return h.astype(np.float32)


def dynamic_stream(M):
    """test_syncword_float64.dynamic_range_stream (segments from 2^-20 to 2^10 and 2^-64, noise, exact zeros, impulses)
    followed by unit impulses at frame offsets 0, 1, M - 1 with silence between them, and an incomplete frame"""
    x = t64.dynamic_range_stream()
    tail = np.zeros(120 * M + M // 2 + 1, np.complex64)
    for i, off in enumerate((0, 1, M - 1)):
        tail[(5 + 35 * i) * M + off] = 1.0 + 0.5j
    return np.concatenate([x, tail])


def run(pkg, x, M, P, taps, cuts=None, **kw):
    """the stream through one handle in one call, or cut at `cuts`; [rows, frames] on the host"""
    import torch
    ch = pkg.Channelizer(M, taps=taps, max_frames=max(x.size // M + 1, 1), **kw)
    xd = dev(x)
    parts, lo = [], 0
    for hi in list(cuts or []) + [x.size]:
        want = ch.output_items(hi - lo)
        parts.append(ch.process_bulk(xd[lo:hi]))
        assert parts[-1].shape[1] == want
        lo = hi
    return host(torch.cat(parts, dim=1))


def ratio(y, y64, x, h, M, P):
    """|y - y64| / (2^-24 sum|h| max|x| over the window); items whose window is all zeros must be exactly zero"""
    wm = cref.window_max(x, M, P)
    scale = cref.EPS32 * np.sum(np.abs(h.astype(np.float64))) * wm
    err = np.abs(y.astype(np.complex128) - y64)
    assert np.all(err[:, scale == 0] == 0)
    nz = scale > 0
    return err[:, nz] / scale[nz][None, :]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("M,P", SIZES)
def test_against_float64(pkg, M, P):
    """every output item within C = P + 5 log2 M of the float64 polyphase form (pinned to the definition by
    tests/test_channelizer_ref.py), the default design and a random prototype.  Measured on MI355X (max / rms of the
    ratio, default design): see DESIGN.md section 14"""
    x = dynamic_stream(M)
    Cb = P + 5 * np.log2(M)
    for name, h in (("default", pkg.channelizer_taps(M, P)), ("random", random_taps(M, P, 3))):
        y64 = cref.analysis64_polyphase(x, h.astype(np.float64), M)
        y = run(pkg, x, M, P, h)
        assert y.shape == y64.shape == (M, x.size // M)
        r = ratio(y, y64, x, h, M, P)
        print(f"\n[channelizer float64] M = {M}, P = {P}, {name} taps: max ratio {r.max():.3f}, rms {np.sqrt(np.mean(r ** 2)):.4f}"
              f" (C = {Cb:.0f})")
        assert r.max() <= Cb
        assert np.max(np.abs(y64)) > 50.0  # the stimulus: the 2^10 segment reaches the output (2^3 alone stays under 10)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("M,P", [(64, 12), (16, 12), (256, 8), (8, 3), (1024, 3), (2, 1)])
def test_one_call_equals_any_chain_of_calls(pkg, M, P):
    L = M * P
    rng = np.random.default_rng(M + P)
    n = 300 * M + M // 2 + 3 if M <= 64 else 40 * M + 5
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    h = random_taps(M, P, 1)
    one = run(pkg, x, M, P, h)
    assert one.shape == (M, n // M)
    steps = [0, 1, M - 1, M, M + 1, L - 1, 0, 0, 1, 1, 2 * M - 1, 3]
    cuts, pos = [], 0
    for s in steps + [int(v) for v in rng.integers(0, 3 * M, 40)] + [int(v) for v in rng.integers(0, 9 * L, 6)]:
        if pos + s <= n:
            pos += s
            cuts.append(pos)
    assert len(cuts) > 30
    assert np.array_equal(bits(run(pkg, x, M, P, h, cuts)), bits(one))


def test_short_calls_of_mixed_formats_equal_one_call(pkg):
    """the history kernel's hard case: calls of 1, 2, 7, 3, 64, 1, ... samples against a tail of 16 to 23, so that most
    of a new tail comes from the old one and the boundary between the old tail and the call's input falls inside it,
    the calls by turns complex64, sc16, sc8 and cu8 forms that unpack exactly to the stream: bit for bit what one
    complex64 call on a fresh handle gives"""
    M, P = 8, 3
    x, forms = exact_iq_forms(624, 32)
    h = random_taps(M, P, 7)
    one = run(pkg, x, M, P, h)
    got = short_calls_of_mixed_formats(pkg, pkg.Channelizer(M, taps=h), x, forms)
    assert one.shape == got.shape == (M, x.size // M)
    assert np.array_equal(bits(got), bits(one))
    assert np.all(np.max(np.abs(one), axis=1) > 0)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("M,P", [(64, 12), (256, 8), (8, 32)])
def test_power_of_two_scaling_is_exact(pkg, M, P):
    rng = np.random.default_rng(5)
    n = 200 * M
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    x[50 * M:60 * M] = 0
    h = pkg.channelizer_taps(M, P)
    y0 = run(pkg, x, M, P, h)
    for k in t64.SCALES:
        f = np.float32(2.0 ** k)
        xs = (x * f).astype(np.complex64)
        assert np.array_equal(xs / f, x)
        assert np.array_equal(bits(run(pkg, xs, M, P, h)), bits((y0 * f).astype(np.complex64))), k


@pytest.mark.timeout(300)
def test_selected_rows_stride_reset_and_two_handles(pkg):
    import torch
    M, P = 64, 12
    rng = np.random.default_rng(9)
    n = 500 * M + 17
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    h = pkg.channelizer_taps(M, P)
    full = run(pkg, x, M, P, h)
    F = n // M
    # row subsets, in list order, fast and generic sizes
    sel = [5, 0, 63, 17, 32]
    assert np.array_equal(bits(run(pkg, x, M, P, h, select=sel)), bits(full[sel]))
    assert np.array_equal(bits(run(pkg, x, M, P, h, cuts=[100, 5000, 5001], select=[63])), bits(full[[63]]))
    x8 = x[:900]
    f8 = run(pkg, x8, 8, 3, random_taps(8, 3))
    assert np.array_equal(bits(run(pkg, x8, 8, 3, random_taps(8, 3), select=[7, 2])), bits(f8[[7, 2]]))
    # a caller's tensor with a larger row stride: the packed result, padding untouched
    fill = np.complex64(complex(np.float32(-7.25), np.float32(3.5)))
    big = torch.full((M, F + 45), complex(fill), dtype=torch.complex64, device="cuda")
    ch = pkg.Channelizer(M, taps=h)
    y = ch.process_bulk(dev(x), out=big[:, 5:5 + F + 3])
    assert tuple(y.shape) == (M, F)
    b = host(big)
    assert np.array_equal(bits(b[:, 5:5 + F]), bits(full))
    assert np.all(b[:, :5] == fill) and np.all(b[:, 5 + F:] == fill)
    # reset(): the fresh stream again (the handle above has seen x and carries 17 samples)
    ch.reset()
    assert ch.output_items(M - 1) == 0 and ch.output_items(M) == 1
    assert np.array_equal(bits(host(ch.process_bulk(dev(x)))), bits(full))
    # two handles on two streams at once: what each gives alone
    x2 = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    full2 = run(pkg, x2, M, P, h)
    xa, xb = dev(x), dev(x2)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        c1 = pkg.Channelizer(M, taps=h)
    with torch.cuda.stream(s2):
        c2 = pkg.Channelizer(M, taps=h)
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


@pytest.mark.timeout(300)
@pytest.mark.parametrize("M,P", FAST)
def test_fast_and_generic_forms_agree_bit_for_bit(pkg, monkeypatch, M, P):
    """GR4PM_CHANNELIZER=generic at create runs the generic form at a size the fast form is built for"""
    x = dynamic_stream(M)
    h = random_taps(M, P, 2)
    monkeypatch.delenv("GR4PM_CHANNELIZER", raising=False)
    fast = run(pkg, x, M, P, h)
    monkeypatch.setenv("GR4PM_CHANNELIZER", "generic")
    generic = run(pkg, x, M, P, h, cuts=[777, 100000])
    assert np.array_equal(bits(fast), bits(generic))
    monkeypatch.setenv("GR4PM_CHANNELIZER", "neither")
    with pytest.raises(pkg.Gr4pmError, match="GR4PM_CHANNELIZER"):
        pkg.Channelizer(M, taps=h)


@pytest.mark.timeout(600)
def test_wideband_to_packets_end_to_end(pkg):
    """M = 64, 20 occupied channels (neighbours, the wrap-around pair 0 / 63), bursts of distinct random payloads from
    PacketTransmitter, a CFO of its own per channel, noise of sigma 0.05 on the wideband stream, synthesised on the GPU
    in complex128; Channelizer (four unequal calls) -> NativeMultiChannelReceiver: per channel as many detector tags as
    bursts, each within one item of where the same receiver finds them in the float64 reference's output; none in an
    empty channel.  Rows 0, 63 and 21 through NativePacketReceiver: every payload byte for byte.  syncword_threshold is
    20.0 as in tests/test_channelizer_ref.py (the default 9.5 fires on rows of noise alone).  The noise seed is 5: with
    seed 4 the detector put one more tag on row 40 at the stream's very first lag (index 1537, noise alone, its median
    history still empty) -- in the float64 reference's output exactly as in the kernel's, so a property of the stimulus;
    the stimulus was changed, not the assertion."""
    import torch
    M, P, N = 64, 12, 30000
    occupied = [0, 1, 2, 63, 62, 10, 11, 20, 21, 22, 30, 31, 32, 33, 40, 45, 46, 50, 55, 56]
    assert len(occupied) == 20
    rng = np.random.default_rng(2025)
    h = pkg.channelizer_taps(M, P)
    hd = torch.from_numpy(h.astype(np.float64)).cuda().reshape(P, M) * M
    tx = pkg.PacketTransmitter()
    r = torch.arange(M, device="cuda", dtype=torch.float64)
    x = torch.zeros((N, M), dtype=torch.complex128, device="cuda")
    sent = {}
    for j, k in enumerate(occupied):
        payloads = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(30, 200, 3)]
        gaps = [int(g) for g in rng.integers(2500, 4000, 3)]
        tx.reset()
        v, _, _ = tx.process_bulk(payloads, gaps=gaps)
        assert v.numel() + 9000 < N
        cfo = float(rng.uniform(-0.03, 0.03))  # rad / item; the detector's +-4 bins reach +-0.042
        v = v.to(torch.complex128) * torch.exp(1j * cfo * torch.arange(v.numel(), device="cuda", dtype=torch.float64))
        vp = torch.zeros(N + P - 1, dtype=torch.complex128, device="cuda")
        vp[P - 1:P - 1 + v.numel()] = v
        s = torch.zeros((N, M), dtype=torch.complex128, device="cuda")
        for p in range(P):  # zero-stuff by M and filter with M h: branch r of frame n takes h[p M + r] v[n - p]
            s += hd[p][None, :] * vp[P - 1 - p:P - 1 - p + N, None]
        x += s * torch.exp(2j * np.pi * ((k * r) % M) / M)[None, :]  # to +k fs / M: exp(2 pi j k (n M + r) / M)
        sent[k] = payloads
    g = torch.Generator(device="cuda").manual_seed(5)
    noise = torch.randn((N, M, 2), dtype=torch.float64, device="cuda", generator=g)
    x = x + (0.05 / np.sqrt(2.0)) * torch.view_as_complex(noise)
    x32 = x.reshape(-1).to(torch.complex64).contiguous()
    torch.cuda.synchronize()

    ch = pkg.Channelizer(M, taps=h)
    parts, lo = [], 0
    for hi in (M * 7000 + 13, M * 7000 + 14, M * 19000 - 1, N * M):
        parts.append(ch.process_bulk(x32[lo:hi]))
        lo = hi
    y = torch.cat(parts, dim=1).contiguous()
    assert tuple(y.shape) == (M, N)
    y64 = cref.analysis64_polyphase(host(x32), h.astype(np.float64), M).astype(np.complex64)
    yr = dev(y64)

    got = pkg.NativeMultiChannelReceiver(M, syncword_threshold=20.0, max_items=N).process_bulk(y)
    ref = pkg.NativeMultiChannelReceiver(M, syncword_threshold=20.0, max_items=N).process_bulk(yr)
    for k in range(M):
        a, b = got[k]["detector_tags"]["index"].astype(np.int64), ref[k]["detector_tags"]["index"].astype(np.int64)
        want = len(sent[k]) if k in sent else 0
        assert a.size == want and b.size == want, (k, a, b)
        assert np.all(np.abs(a - b) <= 1), (k, a, b)
    for k in (21, 0, 63):
        rx = pkg.NativePacketReceiver(max_items=N, tags_cap=2048, syncword_threshold=20.0, decode_headers=True,
                                      packets_only=True)
        assert received_packets(rx.process_bulk(y[k].contiguous())) == sent[k], k


def test_error_paths_return_statuses(pkg):
    import torch
    L = pkg.lib()
    M, P = 64, 12
    with pytest.raises(pkg.Gr4pmError, match="duplicate"):
        pkg.Channelizer(M, select=[3, 3])
    with pytest.raises(pkg.Gr4pmError, match="not a channel"):
        pkg.Channelizer(M, select=[64])
    with pytest.raises(pkg.Gr4pmError):
        pkg.Channelizer(48)
    ch = pkg.Channelizer(M, taps_per_branch=P, max_frames=100)
    x = torch.zeros(101 * M, dtype=torch.complex64, device="cuda")
    out = torch.zeros((M, 128), dtype=torch.complex64, device="cuda")
    n = C.c_size_t(7)
    st = L.gr4pm_channelizer_process(ch._h, x.data_ptr(), 101 * M, out.data_ptr(), 128, 128, C.byref(n))
    assert st == -5 and n.value == 0 and b"made for" in L.gr4pm_last_error()       # beyond max_frames M
    st = L.gr4pm_channelizer_process(ch._h, x.data_ptr(), 50 * M, out.data_ptr(), 128, 49, C.byref(n))
    assert st == -5 and n.value == 0                                                  # out_cap_frames too small
    assert L.gr4pm_channelizer_process(ch._h, None, 50 * M, out.data_ptr(), 128, 128, C.byref(n)) == -1
    assert L.gr4pm_channelizer_process(ch._h, x.data_ptr(), 50 * M, None, 128, 128, C.byref(n)) == -1
    assert L.gr4pm_channelizer_process(ch._h, x.data_ptr(), 50 * M, out.data_ptr(), 128, 128, None) == -1
    assert L.gr4pm_channelizer_process(ch._h, x.data_ptr(), 50 * M, out.data_ptr(), 10, 128, C.byref(n)) == -1
    with pytest.raises(pkg.Gr4pmError):
        ch.process_bulk(x)
    with pytest.raises(pkg.Gr4pmError):
        ch.process_bulk(x[:50 * M], out=out[:, :49])
    # none of the refused calls moved the stream: the handle still is at its start
    assert ch.output_items(M - 1) == 0
    y = ch.process_bulk(x[:50 * M], out=out)
    assert tuple(y.shape) == (M, 50) and n.value == 0
    assert ch.process_bulk(x[:0]).shape[1] == 0
