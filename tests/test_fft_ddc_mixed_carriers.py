"""Two carriers of different symbol rates through one MixedFftDdc, on the GPU: PacketTransmitter bursts at 4 samples per
symbol, one row through Duc([-0.31], 4) and one through Duc([0.17], 16) (a quarter of the symbol rate), summed, plus
noise; MixedFftDdc([-0.31, 0.17], [4, 16]) in one call, a receiver per row fed rows[k, :lengths[k]] delivers every packet
byte for byte; and each row differs from Ddc([f_k], D_k, taps=the same) by no more than the two bounds of
tests/_fft_ddc_mixed_ref.py together (the truncation to two images, the first-order float32 bound).  The handle is tuned
to the set frequencies, not a scan's: a scan bin (1 / 2048) is 0.86 of the detector's pull-in at D = 16 (0.00673 / 16),
too close to assert on; what Spectrum().carriers() finds and what fft_ddc_decimation() makes of the bandwidths is printed.
fft_ddc_decimation() itself is asserted on fixed numbers, without a GPU."""
import numpy as np
import pytest

import _fft_ddc_mixed_ref as mref
import test_spectrum_carriers as scene5
from _frontend import host, received_packets

CARRIERS, DECIMATIONS = [-0.31, 0.17], [4, 16]
BURSTS = [16, 4]
TAIL = 10500  # items of a row behind its last burst: the receiver delivers a packet once the stream goes on well behind it
ROW = [b * (scene5.BURST + scene5.GAP) + TAIL for b in BURSTS]
ROW[0] = ROW[1] * 4  # both rows give the same number of wideband samples
WIDE = ROW[1] * 16
SIGMA = 0.05


def test_fft_ddc_decimation_on_fixed_numbers():
    import __graft_entry__ as ge
    pkg = ge.load_package()
    # the largest power of two <= floor(0.4 / bandwidth): 4, 19, 400, 8, 40, 66, 7, 5
    for bandwidth, want in ((0.084, 4), (0.021, 16), (0.001, 64), (0.05, 8), (0.01, 32), (0.006, 64), (0.055, 4), (0.075, 4)):
        assert pkg.fft_ddc_decimation(bandwidth) == want, bandwidth
        assert want <= pkg.provisional_decimation(bandwidth)
    for bandwidth in (0.2, 0.11, 0.5, 0.0, -1.0, float("nan")):
        with pytest.raises(pkg.Gr4pmError):
            pkg.fft_ddc_decimation(bandwidth)


def row_of_bursts(pkg, n_bursts, n_items, seed):
    """[1, n_items]: n_bursts bursts in test_spectrum_carriers.rows_of_bursts' layout, zeros behind them; and the payloads"""
    import torch
    rng = np.random.default_rng(seed)
    payloads = [rng.integers(0, 256, scene5.PAYLOAD, dtype=np.uint8).tobytes() for _ in range(n_bursts)]
    b, _, _ = pkg.PacketTransmitter().process_bulk(payloads, gaps=[scene5.GAP] * n_bursts)
    assert b.numel() == n_bursts * (scene5.BURST + scene5.GAP) <= n_items - TAIL
    v = torch.zeros((1, n_items), dtype=torch.complex64, device="cuda")
    v[0, :b.numel()] = b
    return v, payloads


@pytest.mark.gpu
def test_two_symbol_rates_through_one_handle():
    from _frontend import load_package
    pkg = load_package()
    assert ROW[0] * 4 == ROW[1] * 16 == WIDE and 200000 <= WIDE <= 400000
    x, sent = None, []
    for k in range(2):
        v, payloads = row_of_bursts(pkg, BURSTS[k], ROW[k], 2027 + k)
        part = pkg.Duc([CARRIERS[k]], DECIMATIONS[k]).process_bulk(v).reshape(-1)
        assert part.numel() == WIDE
        x = part if x is None else x + part
        sent.append(payloads)
    x = pkg.NoiseSource("gaussian", SIGMA, 5, "c64", max_items=WIDE).process_bulk(WIDE, add_to=x).contiguous()

    # printed only: what a scan makes of the scene
    found = pkg.Spectrum().process_bulk(x).carriers()
    for c in found:
        try:
            d = pkg.fft_ddc_decimation(float(c["bandwidth"]))
        except pkg.Gr4pmError as e:
            d = str(e)
        print(f"found carrier frequency {float(c['frequency']):.6f} bandwidth {float(c['bandwidth']):.6f} -> decimation {d}")

    taps = [pkg.fft_ddc_taps(D) for D in DECIMATIONS]
    b = pkg.MixedFftDdc(CARRIERS, DECIMATIONS)
    assert b.overlap == mref.default_overlap(DECIMATIONS, [t.size for t in taps]) == 256
    rows, lengths = b.process_bulk(x)
    S = mref.segments(WIDE, DECIMATIONS, b.overlap)
    assert list(lengths) == [S * b.hop // D for D in DECIMATIONS] and tuple(rows.shape) == (2, int(lengths.max()))
    for k in range(2):
        assert ROW[k] - lengths[k] <= b.hop // DECIMATIONS[k]
        rx = pkg.NativePacketReceiver(max_items=ROW[k], tags_cap=2048, syncword_threshold=20.0, decode_headers=True, packets_only=True)
        assert received_packets(rx.process_bulk(rows[k, :lengths[k]].contiguous())) == sent[k], k

    xs, got = host(x), host(rows)
    truncation = mref.truncation_bound(xs, taps, DECIMATIONS, CARRIERS, b.overlap, 2)
    device = mref.device_bound(xs, taps, DECIMATIONS, CARRIERS, b.overlap, 2)
    for k, D in enumerate(DECIMATIONS):
        ddc = host(pkg.Ddc([CARRIERS[k]], D, taps=taps[k], max_frames=WIDE // D + 1).process_bulk(x))[0, :lengths[k]]
        bound = np.repeat(truncation[k], b.hop // D) + device[k]
        err = np.abs(got[k, :lengths[k]].astype(np.complex128) - ddc.astype(np.complex128))
        print(f"D {D}: MixedFftDdc against Ddc: worst difference / bound {np.max(err / bound):.4f}, worst difference "
              f"{np.max(err):.3e} of {np.max(np.abs(ddc)):.3f}")
        assert np.all(err <= bound), k
        assert not np.any(got[k, lengths[k]:].view(np.float32))
