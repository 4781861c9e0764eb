"""apps/packet_transmitter_file.py with --tune and an integer --format (its function, in process): the Duc or the FftDuc
behind the transmitter writes the file's integers itself.  The file's bytes and the reported
clipped count equal pkg.iq_pack() of the complex64 band, which the test builds from the same blocks called one after the
other: PacketTransmitter, the bank with its tail, iq_pack.  The gains are about twice the defaults, so that a burst of
unit amplitude clips at its peaks."""
import importlib.util
import os

import numpy as np
import pytest

from _frontend import host, load_package

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNE, GAP = 0.13, 500


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def txa():
    spec = importlib.util.spec_from_file_location("packet_transmitter_file", os.path.join(ROOT, "apps", "packet_transmitter_file.py"))
    app = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(app)
    return app


def band(pkg, packets, interpolate, fft_duc):
    """the wideband complex64 stream of the app's chain, block by block"""
    import torch
    tx = pkg.PacketTransmitter(stream_mode=False, samples_per_symbol=4, max_packets=4096, max_payload_bytes=sum(len(p) for p in packets))
    x, _, _ = tx.process_bulk(packets, gaps=[GAP] * len(packets))
    if fft_duc:
        bank = pkg.FftDuc([TUNE], interpolate[0])
        return torch.cat([bank.process_bulk(x), bank.flush()])
    bank = pkg.Duc([TUNE], interpolate[0], decimation=interpolate[1])
    tail = torch.zeros(len(bank.taps) // bank.interpolation + 1, dtype=torch.complex64, device="cuda")
    return torch.cat([bank.process_bulk(x), bank.process_bulk(tail)])


@pytest.mark.parametrize("interpolate,fmt,gain,fft_duc", [((5, 1), "sc16", 60000.0, False), ((25, 4), "cu8", 200.0, False),
                                                          ((4, 1), "sc8", 200.0, True)],
                         ids=["5_sc16", "25over4_cu8", "fft_4_sc8"])
def test_the_file_is_the_band_packed(pkg, txa, tmp_path, interpolate, fmt, gain, fft_duc):
    import torch
    rng = np.random.default_rng(2031)
    packets = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (64, 100, 31)]
    wide = band(pkg, packets, interpolate, fft_duc)
    c = torch.zeros(1, dtype=torch.int64, device="cuda")
    want = host(pkg.iq_pack(wide, fmt, gain, clipped=c))
    path, stats = str(tmp_path / ("wideband." + fmt)), {}
    written = txa.transmit(packets, path, gap=GAP, pkg=pkg, fmt=fmt, gain=gain, stats=stats, tune=TUNE, interpolate=interpolate,
                           fft_duc=fft_duc)
    assert written == wide.numel() == want.shape[0]
    assert open(path, "rb").read() == want.tobytes()
    assert stats["clipped"] == int(c.item())
