"""The channel between the native transmitter and receiver: test/qa_loopback.cpp restated with the native
NoiseSource (bit-exact with the reference's stream), and Channel (apps/packet_transceiver.cpp:48-78) against its
pieces run separately."""
import os
import sys

import numpy as np
import pytest
import torch

import _noise_ref as nr
import _oracle as orc
from test_packet_transmitter import RefTx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

pytestmark = pytest.mark.gpu

# qa_loopback.cpp:30-50: 15 packets of iota bytes (uint8, so wrapping at 256); the last one is too long to get
# through the decoder before the stream ends
QA_LENGTHS = [10, 25, 100, 1500, 27, 38, 243, 514, 1500, 1500, 1024, 1024, 42, 34, 4096]


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return ge.load_package()


@pytest.fixture(scope="module")
def noise_tool(tmp_path_factory):
    return nr.build_stream_tool(str(tmp_path_factory.mktemp("noise")))


def received_packets(r):
    data, lens = r["packets"].cpu().numpy(), r["packet_lengths"]
    got, pos = [], 0
    for n in lens[lens > 0]:
        got.append(data[pos:pos + int(n)].tobytes())
        pos += int(n)
    return got


@pytest.mark.parametrize("stream_mode", [False, True])
@pytest.mark.parametrize("cfo", [0.0, 0.006, -0.02])
def test_qa_loopback_restated(pkg, noise_tool, cfo, stream_mode):
    payloads = [bytes((np.arange(n) % 256).astype(np.uint8)) for n in QA_LENGTHS]
    x, _, _ = pkg.PacketTransmitter(stream_mode=stream_mode, max_packets=16).process_bulk(payloads)
    n = x.numel()
    y = pkg.Rotator(np.float32(cfo)).process_bulk(x)
    noise = pkg.NoiseSource("gaussian", 0.05, 0, "c64", max_items=n)  # qa_loopback.cpp:66-67, seed 0
    z = noise.process_bulk(n, add_to=y)
    # the receiver's input is the reference test's own stimulus: TX restated from the oracle's pieces, the oracle's
    # rotator, the noise restatement, Add(signal, noise)
    m = min(n, 1 << 16)
    tx_ref, _ = RefTx(pkg, 4, stream_mode).process(payloads)
    want = orc.rotator(tx_ref[:m], np.float32(cfo)) + nr.long_stream(noise_tool, "c64", "gaussian", 0, "0.05", m)
    torch.cuda.synchronize()
    assert z[:m].cpu().numpy().tobytes() == want.astype(np.complex64).tobytes()
    for packets_only in (False, True):
        rx = pkg.NativePacketReceiver(max_items=n, tags_cap=2048, decode_headers=True, packets_only=packets_only)
        got = received_packets(rx.process_bulk(z))
        assert got[:14] == payloads[:14], (packets_only, [len(g) for g in got])
        assert len(got) <= 15
        if len(got) == 15:
            assert got[14] == payloads[14]


@pytest.mark.parametrize("sfo_ppm,cfo", [(50.0, 0.003), (-120.0, -0.01)])
def test_channel_equals_its_pieces_across_cuts(pkg, sfo_ppm, cfo):
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(300000, dtype=torch.complex64, device="cuda", generator=g)
    ch = pkg.Channel(samples_per_symbol=4, esn0_db=10.0, cfo=cfo, sfo_ppm=sfo_ppm, seed=3)
    rate = float(np.float32(1.0) + np.float32(1e-6) * np.float32(sfo_ppm))
    assert ch.rate == rate
    amp = float(np.float32(np.sqrt(0.32 * 4 * 10.0 ** -1.0)))
    assert ch.noise_amplitude == amp
    # the pieces, one call each
    r, _ = pkg.PfbArbResampler(rate=rate).process_bulk(x)
    r = pkg.Rotator(np.float32(cfo)).process_bulk(r.contiguous())
    want = pkg.NoiseSource("gaussian", amp, 3, "c64").process_bulk(r.numel(), add_to=r)
    # the channel, in ragged calls
    parts, lo = [], 0
    for hi in (1, 1000, 1001, 77777, 200000, x.numel()):
        parts.append(ch.process_bulk(x[lo:hi].contiguous()))
        lo = hi
    got = torch.cat(parts)
    k = min(got.numel(), want.numel())
    assert k > x.numel() * 0.99
    torch.cuda.synchronize()
    assert got[:k].cpu().numpy().tobytes() == want[:k].cpu().numpy().tobytes()
