"""PacketTransmitter (gr4pm_packet_transmitter, csrc/packet_transmitter.hip) against a restatement of
PacketTransmitterPdu (packet_transmitter_pdu.hpp:40-355) built from the oracle's pinned pieces: CRC, header formatter
and FEC encoder, scrambler and interpolating FIR, plus a numpy GLFSR (glfsr_source.hpp:93-101) and float32 ramps."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

pytestmark = pytest.mark.gpu

GLFSR_MASK_32 = 0x80000057  # x^32 + x^7 + x^5 + x^3 + x^2 + x + 1, glfsr_source.hpp:72
CRC32 = dict(num_bits=32, poly=0x4C11DB7, initial_value=0xFFFFFFFF, final_xor=0xFFFFFFFF, input_reflected=1,
             result_reflected=1)


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return ge.load_package()


class RefTx:
    """packet_transmitter_pdu.hpp restated on the host"""

    def __init__(self, pkg, sps=4, stream_mode=False):
        self.sps, self.stream_mode = sps, stream_mode
        self.gen = np.fromfile(os.path.join(ROOT, "gr4-packet-modem_amd", "data", "header_ldpc_generator.u32"), dtype="<u4")
        self.taps = pkg.packet_transmitter_rrc_taps(sps)
        self.glfsr = 1
        a = np.float32(np.sqrt(np.float32(2.0)) / np.float32(2.0))
        self.qpsk = np.array([a + 1j * a, a - 1j * a, -a + 1j * a, -a - 1j * a], dtype=np.complex64)
        self.sync = np.where(pkg.SYNCWORD == 1, -1.0, 1.0).astype(np.complex64)
        n_lead, n_trail = 8 * sps, 11 * sps
        self.lead = np.array([math.sin((j + 1) / n_lead * 0.5 * math.pi) for j in range(n_lead)], dtype=np.float32)
        self.trail = np.array([math.sin((j + 1) / n_trail * 0.5 * math.pi) for j in range(n_trail)][::-1], dtype=np.float32)
        self.fir = orc.InterpolatingFir(sps, self.taps)

    def glfsr_bits(self, n):
        out = np.empty(n, dtype=np.uint8)
        r = self.glfsr
        for i in range(n):
            out[i] = r & 1
            r = (r >> 1) ^ (GLFSR_MASK_32 if r & 1 else 0)
        self.glfsr = r
        return out

    def symbols(self, data, ptype=0):
        d = np.frombuffer(bytes(data), dtype=np.uint8)
        crc = orc.crc_compute(d, **CRC32)
        hdr = orc.header_fec_encode(orc.header_format(d.size, ptype), self.gen)[0]
        bits = np.unpackbits(np.concatenate([hdr, d, np.frombuffer(crc.to_bytes(4, "big"), dtype=np.uint8)]))
        scr = orc.AdditiveScrambler(0x4001, 0x18E38, 16).process(bits)
        parts = [self.sync, self.qpsk[scr[0::2] * 2 + scr[1::2]]]
        if not self.stream_mode:
            rb = self.glfsr_bits(18)
            parts += [self.qpsk[rb[0::2] * 2 + rb[1::2]], np.zeros(11, dtype=np.complex64)]
        return np.concatenate(parts)

    def shape(self, x):
        y = x.copy().view(np.float32).reshape(-1, 2)
        nl, nt = self.lead.size, self.trail.size
        y[:nl] *= self.lead[:, None]
        y[-nt:] *= self.trail[:, None]
        return y.reshape(-1).view(np.complex64)

    def process(self, payloads, types=None, gaps=None):
        types = types if types is not None else [0] * len(payloads)
        if self.stream_mode:
            x = self.fir.process(np.concatenate([self.symbols(p, t) for p, t in zip(payloads, types)]))
            return x, None
        parts, lens = [], []
        for k, (p, t) in enumerate(zip(payloads, types)):
            if gaps is not None:
                parts.append(np.zeros(int(gaps[k]), dtype=np.complex64))
            b = self.shape(self.fir.process(self.symbols(p, t)))
            parts.append(b)
            lens.append(b.size)
        return np.concatenate(parts), np.array(lens, dtype=np.uint64)


def bits(x):
    return (x.cpu().numpy() if isinstance(x, torch.Tensor) else x).view(np.int32)


def rand_payloads(rng, lengths):
    return [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in lengths]


CASES = {
    "one": (4, [1]),
    "two": (4, [2, 1500]),
    "edges": (4, [1, 2, 3, 1500, 65535, 7, 64, 65]),
    "thousand": (4, "1000"),
    "sps3": (3, [1, 2, 3, 1500, 333, 64, 19]),
    "sps2": (2, [3, 1500, 1]),
}


@pytest.mark.parametrize("case", list(CASES))
def test_burst_mode_bit_exact(pkg, case):
    sps, lengths = CASES[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    if lengths == "1000":
        lengths = rng.integers(1, 400, 1000)
    payloads = rand_payloads(rng, lengths)
    types = rng.integers(0, 2, len(payloads))
    tx = pkg.PacketTransmitter(samples_per_symbol=sps, max_packets=1024, max_payload_bytes=1 << 20)
    got, offs, lens = tx.process_bulk(payloads, packet_types=types)
    want, want_lens = RefTx(pkg, sps).process(payloads, types)
    assert np.array_equal(lens, want_lens)
    assert np.array_equal(lens, [sps * (4 * len(p) + 228) for p in payloads])
    assert np.array_equal(offs, np.concatenate([[0], np.cumsum(want_lens)[:-1]]).astype(np.uint64))
    assert got.numel() == want.size and np.array_equal(bits(got), bits(want))


def test_device_tensor_input_equals_list_input(pkg):
    rng = np.random.default_rng(5)
    payloads = rand_payloads(rng, [10, 700, 1])
    a, _, _ = pkg.PacketTransmitter().process_bulk(payloads)
    dev = torch.from_numpy(np.frombuffer(b"".join(payloads), dtype=np.uint8).copy()).cuda()
    b, _, _ = pkg.PacketTransmitter().process_bulk(dev, lengths=[10, 700, 1])
    assert np.array_equal(bits(a), bits(b))


def test_glfsr_continues_across_calls_and_reset(pkg):
    rng = np.random.default_rng(8)
    payloads = rand_payloads(rng, rng.integers(1, 200, 120))
    one, _, _ = pkg.PacketTransmitter().process_bulk(payloads)
    tx = pkg.PacketTransmitter()
    cuts = sorted(set(rng.integers(1, len(payloads), 6).tolist())) + [len(payloads)]
    parts, at = [], 0
    for c in cuts:
        parts.append(tx.process_bulk(payloads[at:c])[0].cpu().numpy())
        at = c
    assert np.array_equal(bits(np.concatenate(parts)), bits(one))
    # the register ran on: the same packets again give other ramp-down symbols ...
    again = tx.process_bulk(payloads[:5])[0]
    first = pkg.PacketTransmitter().process_bulk(payloads[:5])[0]
    assert not np.array_equal(bits(again), bits(first))
    # ... until reset()
    tx.reset()
    assert np.array_equal(bits(tx.process_bulk(payloads[:5])[0]), bits(first))


@pytest.mark.parametrize("sps", [4, 3])
def test_stream_mode_bit_exact_and_cuts(pkg, sps):
    rng = np.random.default_rng(20 + sps)
    payloads = rand_payloads(rng, list(rng.integers(1, 600, 80)) + [1, 2, 3, 1500])
    types = rng.integers(0, 2, len(payloads))
    tx = pkg.PacketTransmitter(stream_mode=True, samples_per_symbol=sps)
    got, offs, lens = tx.process_bulk(payloads, packet_types=types)
    want, _ = RefTx(pkg, sps, stream_mode=True).process(payloads, types)
    assert np.array_equal(lens, [sps * (4 * len(p) + 208) for p in payloads])
    assert np.array_equal(offs, np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64))
    assert np.array_equal(bits(got), bits(want))
    tx = pkg.PacketTransmitter(stream_mode=True, samples_per_symbol=sps)
    cuts = sorted(set(rng.integers(1, len(payloads), 7).tolist())) + [len(payloads)]
    parts, at = [], 0
    for c in cuts:
        parts.append(tx.process_bulk(payloads[at:c], packet_types=types[at:c])[0].cpu().numpy())
        at = c
    assert np.array_equal(bits(np.concatenate(parts)), bits(want))
    tx.reset()
    assert np.array_equal(bits(tx.process_bulk(payloads[:3], packet_types=types[:3])[0]),
                          bits(RefTx(pkg, sps, stream_mode=True).process(payloads[:3], types[:3])[0]))


def test_gaps(pkg):
    rng = np.random.default_rng(12)
    payloads = rand_payloads(rng, rng.integers(1, 300, 40))
    gaps = rng.integers(0, 5000, len(payloads))
    gaps[3] = 0
    gaps[7] = 1
    plain, _, lens = pkg.PacketTransmitter().process_bulk(payloads)
    got, offs, glens = pkg.PacketTransmitter().process_bulk(payloads, gaps=gaps)
    assert np.array_equal(lens, glens)
    want_offs = np.cumsum(gaps) + np.concatenate([[0], np.cumsum(lens)[:-1]])
    assert np.array_equal(offs, want_offs.astype(np.uint64))
    plain = plain.cpu().numpy()
    parts, at = [], 0
    for g, n in zip(gaps, lens):
        parts += [np.zeros(int(g), dtype=np.complex64), plain[at:at + int(n)]]
        at += int(n)
    assert np.array_equal(bits(got), bits(np.concatenate(parts)))
    want, _ = RefTx(pkg).process(payloads, gaps=gaps)
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("packets_only", [False, True])
def test_loopback_through_the_native_receiver(pkg, packets_only):
    rng = np.random.default_rng(300)
    payloads = rand_payloads(rng, rng.integers(1, 1500, 300))
    types = rng.integers(0, 2, len(payloads))
    gaps = rng.integers(1200, 4000, len(payloads))
    x, _, _ = pkg.PacketTransmitter(max_packets=300).process_bulk(payloads, packet_types=types, gaps=gaps)
    x = torch.cat([x, torch.zeros(4000, dtype=torch.complex64, device=x.device)])
    x = pkg.Rotator(np.float32(0.01)).process_bulk(x)
    n0 = 0.32 * 4 * 10.0 ** (-0.1 * 20.0)  # Es/N0 = 20 dB at tx power 0.32, apps/packet_transceiver.cpp:48-52
    g = torch.Generator(device="cuda")
    g.manual_seed(4)
    noise = torch.complex(torch.randn(x.numel(), generator=g, device="cuda"),
                          torch.randn(x.numel(), generator=g, device="cuda")) * np.float32(np.sqrt(n0 / 2.0))
    x = (x + noise).to(torch.complex64)
    rx = pkg.NativePacketReceiver(max_items=x.numel(), tags_cap=2048, decode_headers=True, packets_only=packets_only)
    r = rx.process_bulk(x)
    assert r["header_mismatches"] == 0
    valid = r["header_messages"]["invalid_header"] == 0
    assert list(r["packet_type"][valid]) == list(types)
    data, lens = r["packets"].cpu().numpy(), r["packet_lengths"]
    got, pos = [], 0
    for n in lens[lens > 0]:
        got.append(data[pos:pos + int(n)].tobytes())
        pos += int(n)
    assert got == payloads


def test_refused_inputs_leave_the_output_untouched(pkg):
    tx = pkg.PacketTransmitter(max_packets=4, max_payload_bytes=70000)
    pattern = torch.full((1 << 20,), 3.0 + 4.0j, dtype=torch.complex64, device="cuda")
    ok = [b"\x01" * 10]

    def refused(payloads, **kw):
        out = pattern.clone()
        with pytest.raises(pkg.Gr4pmError):
            tx.process_bulk(payloads, out=out, **kw)
        torch.cuda.synchronize()
        assert torch.equal(out, pattern)

    refused([b"\x00" * 65536])                                   # header_formatter.hpp:102-106
    refused([b"", b"\x01"])                                      # packet_ingress.hpp:171-172
    refused(ok * 5)                                              # max_packets
    refused([b"\x02" * 40000, b"\x02" * 40000])                  # max_payload_bytes
    refused(ok, packet_types=[2])
    out = pattern[: 4 * (40 + 228) - 1].clone()                  # out_cap one short
    with pytest.raises(pkg.Gr4pmError):
        tx.process_bulk(ok, out=out)
    assert torch.equal(out, pattern[: out.numel()])
    with pytest.raises(pkg.Gr4pmError):                          # gaps are a burst mode setting
        pkg.PacketTransmitter(stream_mode=True).process_bulk(ok, gaps=[10])
    # the edges that are accepted: 65535 bytes, exactly out_cap, and nothing refused left its mark on the GLFSR
    x, _, _ = tx.process_bulk([b"\x05" * 65535])
    assert x.numel() == 4 * (4 * 65535 + 228)
    out = pattern[: 4 * (40 + 228)].clone()
    y, _, _ = tx.process_bulk(ok, out=out)
    assert y.numel() == out.numel()
    first = pkg.PacketTransmitter().process_bulk([b"\x05" * 65535] + ok)[0]
    assert np.array_equal(bits(torch.cat([x, y])), bits(first))


def test_app_round_trip(pkg, tmp_path):
    rng = np.random.default_rng(77)
    packets = rand_payloads(rng, rng.integers(1, 1500, 40))
    src = tmp_path / "in.bin"
    with open(src, "wb") as f:
        for p in packets:
            f.write(len(p).to_bytes(2, "big") + p)
    iq, back = tmp_path / "iq.c64", tmp_path / "out.bin"
    env = dict(os.environ)
    subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "apps", "packet_transmitter_file.py"),
                    str(iq), "--in", str(src), "--gap", "3000"], check=True, env=env)
    assert os.path.getsize(iq) == 8 * sum(3000 + 4 * (4 * len(p) + 228) for p in packets)
    with open(iq, "ab") as f:  # silence behind the last burst, as in front of every other one
        f.write(np.zeros(8192, dtype=np.complex64).tobytes())
    subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "apps", "packet_receiver_file.py"),
                    str(iq), "--out", str(back)], check=True, env=env)
    assert back.read_bytes() == src.read_bytes()
