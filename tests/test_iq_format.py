"""Integer IQ on the GPU: gr4pm_iq_unpack / gr4pm_iq_pack byte for byte against tests/_iq_ref.py (every value, every
edge of the vector body at every alignment, rows with gaps, the clipped counter), the channelizer's integer ingest bit
for bit against process() on the unpacked samples, wideband int16 -> Channelizer -> receivers -> payload bytes, and the
two file apps with --format sc16.  No tolerance anywhere: the definition is exact."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _iq_ref as iqr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = list(iqr.FORMATS)
EDGE_N = [0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1023, 4099]
PAD = 64  # sentinel items on either side of an output


@pytest.fixture(scope="module")
def pkg():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import __graft_entry__ as ge
    return ge.load_package()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def random_items(fmt, shape, seed):
    dtype, _, _, lo, hi, _, _ = iqr.FORMATS[fmt]
    return np.random.default_rng(seed).integers(lo, hi + 1, tuple(shape) + (2,)).astype(dtype)


def random_c64(n, seed, sigma=0.5):
    rng = np.random.default_rng(seed)
    return (sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


@pytest.mark.parametrize("fmt", FORMATS)
def test_unpack_every_value(pkg, fmt):
    """sc16: 65 536 items with every int16 as I and the reversed sequence as Q; sc8, cu8: every (I, Q) pair"""
    dtype, _, _, lo, hi, _, _ = iqr.FORMATS[fmt]
    v = np.arange(lo, hi + 1, dtype=np.int64)
    if fmt == "sc16":
        items = np.stack([v, v[::-1]], axis=1).astype(dtype)
    else:
        items = np.stack(np.meshgrid(v, v, indexing="ij"), axis=-1).reshape(-1, 2).astype(dtype)
    assert items.shape == (65536, 2)
    x = dev(items)
    for scale in (None, 1.0, 3.0e-5):
        got = host(pkg.iq_unpack(x, scale))
        assert np.array_equal(bits(got), bits(iqr.unpack(items, fmt, scale))), scale
    # and back: pack of unpack is the identity, nothing clipped
    import torch
    clipped = torch.zeros(1, dtype=torch.int64, device="cuda")
    back = host(pkg.iq_pack(pkg.iq_unpack(x), fmt, clipped=clipped))
    assert np.array_equal(back, items) and int(clipped.item()) == 0


@pytest.mark.parametrize("fmt", FORMATS)
def test_unpack_edges_of_the_vector_body(pkg, fmt):
    import torch
    src = random_items(fmt, (8 + max(EDGE_N),), 11)
    want = iqr.unpack(src, fmt)
    x = dev(src)
    sentinel = np.complex64(complex(np.float32(-7.25), np.float32(3.5)))
    for n in EDGE_N:
        for ioff in range(9):
            for ooff in (0, 1):
                buf = torch.full((PAD + ooff + n + PAD,), complex(sentinel), dtype=torch.complex64, device="cuda")
                y = pkg.iq_unpack(x[ioff:ioff + n], out=buf[PAD + ooff:PAD + ooff + n])
                assert n == 0 or y.data_ptr() == buf.data_ptr() + 8 * (PAD + ooff)
                b = host(buf)
                assert np.array_equal(bits(b[PAD + ooff:PAD + ooff + n]), bits(want[ioff:ioff + n])), (n, ioff, ooff)
                assert np.all(bits(b[:PAD + ooff]) == bits(sentinel)) and np.all(bits(b[PAD + ooff + n:]) == bits(sentinel)), \
                    (n, ioff, ooff)


@pytest.mark.parametrize("fmt", FORMATS)
def test_pack_edges_of_the_vector_body(pkg, fmt):
    """the output offsets 0 and 1 the unpack test takes, and every other offset up to a whole 16-byte line (the head that
    pack peels has up to 3 or 7 items)"""
    import torch
    dtype = iqr.FORMATS[fmt][0]
    src = random_c64(8 + max(EDGE_N), 12, sigma=0.6)  # a few per cent clip
    want, _ = iqr.pack(src, fmt)
    x = dev(src)
    sentinel, tdtype = 0x5A, dev(np.zeros(1, dtype)).dtype
    for n in EDGE_N:
        for ioff in range(9):
            for ooff in (range(9) if ioff in (0, 1) else (0, 1)):
                buf = torch.full((PAD + ooff + n + PAD, 2), sentinel, dtype=tdtype, device="cuda")
                pkg.iq_pack(x[ioff:ioff + n], fmt, out=buf[PAD + ooff:PAD + ooff + n])
                b = host(buf)
                assert np.array_equal(b[PAD + ooff:PAD + ooff + n], want[ioff:ioff + n]), (n, ioff, ooff)
                assert np.all(b[:PAD + ooff] == sentinel) and np.all(b[PAD + ooff + n:] == sentinel), (n, ioff, ooff)


@pytest.mark.parametrize("fmt", FORMATS)
def test_rows_with_strides(pkg, fmt):
    """3 rows of 1000 items at strides of 1003 in and 1001 out, both directions: the gaps stay as they were"""
    import torch
    rows, n, si, so = 3, 1000, 1003, 1001
    src = random_items(fmt, (rows, si), 21)
    fill = complex(np.float32(1.5), np.float32(-2.5))
    out = torch.full((rows, so), fill, dtype=torch.complex64, device="cuda")
    y = pkg.iq_unpack(dev(src)[:, :n], out=out[:, :n])
    assert tuple(y.shape) == (rows, n)
    b = host(out)
    assert np.array_equal(bits(b[:, :n]), bits(iqr.unpack(src[:, :n], fmt)))
    assert np.all(b[:, n:] == np.complex64(fill))
    assert np.array_equal(bits(host(pkg.iq_unpack(dev(src)[:, :n]))), bits(iqr.unpack(src[:, :n], fmt)))  # out=None

    csrc = random_c64(rows * si, 22, sigma=0.6).reshape(rows, si)
    iout = torch.full((rows, so, 2), 0x5A, dtype=dev(src).dtype, device="cuda")
    clipped = torch.zeros(1, dtype=torch.int64, device="cuda")
    z = pkg.iq_pack(dev(csrc)[:, :n], fmt, out=iout[:, :n], clipped=clipped)
    assert tuple(z.shape) == (rows, n, 2)
    want, count = iqr.pack(csrc[:, :n], fmt)
    b = host(iout)
    assert np.array_equal(b[:, :n], want) and np.all(b[:, n:] == 0x5A)
    assert int(clipped.item()) == count and count > 0  # the gaps' items would have been counted too


def special_values(fmt, gain):
    """(k + 0.5) / gain and k / gain for k in -4 .. 4 and around both ends of the range (for cu8: of the range before
    its offset too); infinities, NaN, -0.0, denormals; 10^4 normal deviates x 0.5"""
    _, _, _, lo, hi, bias, _ = iqr.FORMATS[fmt]
    ks = set(range(-4, 5))
    for end in (lo, hi, int(np.floor(lo - bias)), int(np.floor(hi - bias))):
        ks.update(range(end - 4, end + 5))
    ks = np.array(sorted(ks), dtype=np.float32)
    g = np.float32(gain)
    v = np.concatenate([(ks + np.float32(0.5)) / g, ks / g, (ks - np.float32(0.5)) / g,
                        np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, 1e-40, -1e-40, 1.4e-45, 3e38, -3e38], dtype=np.float32)])
    v = v.astype(np.float32)
    rng = np.random.default_rng(31)
    x = np.zeros(2 * v.size + 10000, dtype=np.complex64)
    x.real[:v.size], x.imag[:v.size] = v, v[::-1]              # each special value as I and as Q
    x.real[v.size:2 * v.size], x.imag[v.size:2 * v.size] = 0.25, v
    x.real[2 * v.size:] = 0.5 * rng.standard_normal(10000)
    x.imag[2 * v.size:] = 0.5 * rng.standard_normal(10000)
    return x


@pytest.mark.parametrize("fmt", FORMATS)
def test_pack_values_and_clipped_counter(pkg, fmt):
    import torch
    total = 0
    clipped = torch.zeros(1, dtype=torch.int64, device="cuda")
    for gain in (None, 1000.0):
        x = special_values(fmt, iqr.FORMATS[fmt][2] if gain is None else gain)
        want, count = iqr.pack(x, fmt, gain)
        assert count > 10
        got = host(pkg.iq_pack(dev(x), fmt, gain, clipped=clipped))
        assert got.dtype == want.dtype and np.array_equal(got, want), gain
        total += count
        assert int(clipped.item()) == total                    # the counter accumulates over the calls
        assert np.array_equal(host(pkg.iq_pack(dev(x), fmt, gain)), want)  # clipped=None
    assert int(clipped.item()) == total


CHAN_SIZES = [(64, 12), (16, 12), (256, 8), (8, 3)]


def chan_run(pkg, M, P, h, pieces, scale=None, **kw):
    """a handle of its own; pieces: tensors (complex64 or integer IQ) fed one call each; [rows, frames] on the device"""
    import torch
    ch = pkg.Channelizer(M, taps=h, max_frames=8192, **kw)
    parts = []
    for p in pieces:
        integer = p.dtype != torch.complex64
        parts.append(ch.process_bulk(p, scale=scale) if integer else ch.process_bulk(p))
    return torch.cat(parts, dim=1)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("M,P", CHAN_SIZES)
def test_channelizer_integer_ingest_is_bit_equal(pkg, monkeypatch, M, P, fmt):
    import torch
    monkeypatch.delenv("GR4PM_CHANNELIZER", raising=False)
    n_in = 3 * 4096 + 37  # three workgroups and a partial frame
    items = random_items(fmt, (n_in,), 100 + M)
    xi = dev(items)
    h = pkg.channelizer_taps(M, P)
    for scale in (None, 3.0e-5):
        xc = pkg.iq_unpack(xi, scale)
        assert np.array_equal(bits(host(xc)), bits(iqr.unpack(items, fmt, scale)))
        ref = host(chan_run(pkg, M, P, h, [xc]))
        assert ref.shape == (M, n_in // M) and np.any(ref != 0)
        assert np.array_equal(bits(host(chan_run(pkg, M, P, h, [xi], scale))), bits(ref)), scale
    # (from here on: scale, xc and ref of the loop's last pass, 3.0e-5)
    cuts, pos = [], 0
    for step in (0, 1, M - 1, M + 1, 4097):
        cuts.append((pos, pos + step))
        pos += step
    cuts.append((pos, n_in))
    assert np.array_equal(bits(host(chan_run(pkg, M, P, h, [xi[a:b] for a, b in cuts], scale))), bits(ref))
    # one handle fed a complex64 call and then an integer call: the complex64 handle on the concatenation
    pre = dev(random_c64(5 * M + 3, 7, sigma=0.3))
    both = host(chan_run(pkg, M, P, h, [torch.cat([pre, xc])]))
    assert np.array_equal(bits(host(chan_run(pkg, M, P, h, [pre, xi], scale))), bits(both))
    assert np.array_equal(bits(host(chan_run(pkg, M, P, h, [xi[:1000], xc[1000:5000], xi[5000:]], scale))), bits(ref))
    # selected rows into a caller's tensor with a larger row stride
    sel = [M - 1, 0, 3]
    F = n_in // M
    fill = complex(np.float32(-7.25), np.float32(3.5))
    big = torch.full((len(sel), F + 9), fill, dtype=torch.complex64, device="cuda")
    ch = pkg.Channelizer(M, taps=h, select=sel, max_frames=8192)
    y = ch.process_bulk(xi, out=big[:, 2:2 + F + 1], scale=scale)
    assert tuple(y.shape) == (len(sel), F)
    b = host(big)
    assert np.array_equal(bits(b[:, 2:2 + F]), bits(ref[sel]))
    assert np.all(b[:, :2] == np.complex64(fill)) and np.all(b[:, 2 + F:] == np.complex64(fill))
    # the generic form at the same size
    monkeypatch.setenv("GR4PM_CHANNELIZER", "generic")
    assert np.array_equal(bits(host(chan_run(pkg, M, P, h, [xi[:4097], xi[4097:]], scale))), bits(ref))
    assert np.array_equal(bits(host(chan_run(pkg, M, P, h, [pre, xi], scale))), bits(both))


def received_packets(r):
    data, lens = r["packets"].cpu().numpy(), r["packet_lengths"]
    got, pos = [], 0
    for n in lens[lens > 0]:
        got.append(data[pos:pos + int(n)].tobytes())
        pos += int(n)
    return got


@pytest.mark.timeout(600)
def test_wideband_int16_to_packets_end_to_end(pkg):
    """the wideband signal of test_channelizer.py's end-to-end test (M = 64, 20 occupied channels, three bursts each, a
    CFO per channel, noise of sigma 0.05), packed to sc16 at half of full scale: Channelizer on the int16 tensor ->
    NativeMultiChannelReceiver finds every burst and nothing else, and rows 21, 0 and 63 through NativePacketReceiver
    give every payload byte for byte, as the complex64 path does."""
    import torch
    M, P, N = 64, 12, 30000
    occupied = [0, 1, 2, 63, 62, 10, 11, 20, 21, 22, 30, 31, 32, 33, 40, 45, 46, 50, 55, 56]
    rng = np.random.default_rng(2025)
    h = pkg.channelizer_taps(M, P)
    hd = torch.from_numpy(h.astype(np.float64)).cuda().reshape(P, M) * M
    tx = pkg.PacketTransmitter()
    r = torch.arange(M, device="cuda", dtype=torch.float64)
    x = torch.zeros((N, M), dtype=torch.complex128, device="cuda")
    sent = {}
    for k in occupied:
        payloads = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(30, 200, 3)]
        gaps = [int(g) for g in rng.integers(2500, 4000, 3)]
        tx.reset()
        v, _, _ = tx.process_bulk(payloads, gaps=gaps)
        assert v.numel() + 9000 < N
        cfo = float(rng.uniform(-0.03, 0.03))
        v = v.to(torch.complex128) * torch.exp(1j * cfo * torch.arange(v.numel(), device="cuda", dtype=torch.float64))
        vp = torch.zeros(N + P - 1, dtype=torch.complex128, device="cuda")
        vp[P - 1:P - 1 + v.numel()] = v
        s = torch.zeros((N, M), dtype=torch.complex128, device="cuda")
        for p in range(P):
            s += hd[p][None, :] * vp[P - 1 - p:P - 1 - p + N, None]
        x += s * torch.exp(2j * np.pi * ((k * r) % M) / M)[None, :]
        sent[k] = payloads
    g = torch.Generator(device="cuda").manual_seed(5)
    noise = torch.randn((N, M, 2), dtype=torch.float64, device="cuda", generator=g)
    x = x + (0.05 / np.sqrt(2.0)) * torch.view_as_complex(noise)
    x32 = x.reshape(-1).to(torch.complex64).contiguous()

    peak = float(torch.view_as_real(x32).abs().max().item())
    gain = 0.5 * 32768.0 / peak  # the largest component at half of full scale
    clipped = torch.zeros(1, dtype=torch.int64, device="cuda")
    x16 = pkg.iq_pack(x32, "sc16", gain, clipped=clipped)
    assert x16.dtype == torch.int16 and tuple(x16.shape) == (N * M, 2) and int(clipped.item()) == 0
    assert 16000 <= int(x16.abs().max().item()) <= 16384

    def channels(samples, **kw):
        ch = pkg.Channelizer(M, taps=h)
        parts, lo = [], 0
        for hi in (M * 7000 + 13, M * 7000 + 14, M * 19000 - 1, N * M):
            parts.append(ch.process_bulk(samples[lo:hi], **kw))
            lo = hi
        return torch.cat(parts, dim=1).contiguous()

    paths = {"sc16": channels(x16, scale=1.0 / gain), "complex64": channels(x32)}
    for name, y in paths.items():
        assert tuple(y.shape) == (M, N)
        got = pkg.NativeMultiChannelReceiver(M, syncword_threshold=20.0, max_items=N).process_bulk(y)
        for k in range(M):
            assert got[k]["detector_tags"].size == (len(sent[k]) if k in sent else 0), (name, k)
        for k in (21, 0, 63):
            rx = pkg.NativePacketReceiver(max_items=N, tags_cap=2048, syncword_threshold=20.0, decode_headers=True,
                                          packets_only=True)
            assert received_packets(rx.process_bulk(y[k].contiguous())) == sent[k], (name, k)


def test_apps_round_trip_sc16(tmp_path):
    """packet_transmitter_file.py --format sc16 into packet_receiver_file.py --format sc16, as child processes"""
    rng = np.random.default_rng(1)  # the app's --seed default
    packets = [rng.integers(0, 256, 200, dtype=np.uint8).tobytes() for _ in range(8)]
    iq, back = tmp_path / "iq.sc16", tmp_path / "out.bin"
    env = dict(os.environ)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "apps", "packet_transmitter_file.py"),
                        str(iq), "--random", "8", "200", "--gap", "4000", "--format", "sc16"], check=True, env=env,
                       capture_output=True, text=True)
    m = re.search(r"(\d+) clipped components", r.stdout)
    assert m and int(m.group(1)) == 0, r.stdout
    assert os.path.getsize(iq) == 4 * 8 * (4000 + 4 * (4 * 200 + 228))
    with open(iq, "ab") as f:  # silence behind the last burst, as in front of every other one
        f.write(np.zeros((8192, 2), dtype=np.int16).tobytes())
    subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "apps", "packet_receiver_file.py"),
                    str(iq), "--format", "sc16", "--out", str(back)], check=True, env=env)
    assert back.read_bytes() == b"".join(len(p).to_bytes(2, "big") + p for p in packets)
