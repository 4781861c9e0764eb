"""Two carriers whose symbols are no 4 * 2^k wideband samples long, received as a stream, on the GPU: PacketTransmitter
bursts at 4 samples per symbol, one row through Duc([-0.31], 5) (20 wideband samples per symbol) and one through
Duc([0.17], 25, decimation=4) (25 per symbol), summed, plus noise of 0.05.  MixedFftDdc -> StreamRowResampler.for_rates(the
true rates) -> RowPacketReceivers, fed in calls of 1, of 4097, of 65 536 and of all samples: every payload of both carriers
arrives byte for byte in all four runs, and the resampler's concatenated output is the same bytes in all four.

The run in calls of one sample makes 330 000 calls of MixedFftDdc.process_bulk; the blocks behind it are called whenever it
delivers frames (a call without frames changes nothing in them)."""
import numpy as np
import pytest

import test_spectrum_carriers as scene5
from _frontend import load_package
from test_fft_ddc_mixed_carriers import TAIL, row_of_bursts

pytestmark = pytest.mark.gpu

CARRIERS = [-0.31, 0.17]
WIDE = 330000
ROW = [WIDE // 5, WIDE * 4 // 25]  # items of the transmit rows at 4 samples per symbol
PER_SYMBOL = [20, 25]              # wideband samples
BURSTS = [16, 12]
SIGMA = 0.05
CALLS = [1, 4097, 65536, WIDE]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def scene(pkg):
    return build_scene(pkg)


def build_scene(pkg):
    """(the wideband stream, the payloads per carrier)"""
    assert ROW[0] * 5 == WIDE and ROW[1] * 25 == WIDE * 4
    x, sent = None, []
    for k, duc in enumerate((pkg.Duc([CARRIERS[0]], 5), pkg.Duc([CARRIERS[1]], 25, decimation=4))):
        assert BURSTS[k] * (scene5.BURST + scene5.GAP) + TAIL <= ROW[k]
        v, payloads = row_of_bursts(pkg, BURSTS[k], ROW[k], 2029 + k)
        part = duc.process_bulk(v).reshape(-1)
        assert part.numel() == WIDE
        x = part if x is None else x + part
        sent.append(payloads)
    x = pkg.NoiseSource("gaussian", SIGMA, 5, "c64", max_items=WIDE).process_bulk(WIDE, add_to=x).contiguous()
    return x, sent


def receive(pkg, x, call, decimations):
    """the chain over x in calls of `call` samples: (packets per carrier, the resampler's output per carrier)"""
    import torch
    rates = [D / s for D, s in zip(decimations, PER_SYMBOL)]  # symbols per row item
    ddc = pkg.MixedFftDdc(CARRIERS, decimations)
    rs = pkg.StreamRowResampler.for_rates(rates, max_step=1.6)
    rx = pkg.RowPacketReceivers(2, syncword_threshold=20.0)
    packets, items = [[], []], [[], []]

    def behind(y, m):
        for k in range(2):
            items[k].append(y[k, :int(m[k])].clone())
        for k, got in enumerate(rx.process_rows(y, m)):
            packets[k] += got

    for lo in range(0, WIDE, call):
        rows, lengths = ddc.process_bulk(x[lo:lo + call])
        if lengths.any():
            behind(*rs.process_rows(rows, lengths))
    behind(*rs.flush())
    for k, got in enumerate(rx.flush()):
        packets[k] += got
    torch.cuda.synchronize()
    return packets, [torch.cat(i).cpu().numpy() for i in items]


def test_two_carriers_of_odd_rates_in_any_cutting(pkg, scene):
    x, sent = scene
    decimations = [pkg.fft_ddc_decimation(1.35 / s) for s in PER_SYMBOL]  # the occupied band of a root-raised cosine of 0.35
    assert decimations[0] == 4 and decimations[1] in (4, 8)
    first = None
    for call in CALLS:
        packets, items = receive(pkg, x, call, decimations)
        for k in range(2):
            assert packets[k] == sent[k], (call, k, len(packets[k]), len(sent[k]))
        if first is None:
            first = items
            for k in range(2):  # 4 samples per symbol: the transmit row's length, less what the Ddc still holds
                print(f"carrier {k}: decimation {decimations[k]}, {items[k].size} items at 4 samples per symbol of {ROW[k]}")
                assert 0 <= ROW[k] - items[k].size <= 2048 * 4 // PER_SYMBOL[k] + 64
        for k in range(2):
            assert items[k].tobytes() == first[k].tobytes(), (call, k)
