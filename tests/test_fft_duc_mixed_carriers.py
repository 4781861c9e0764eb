"""Two carriers of different symbol rates from one MixedFftDuc and back through one MixedFftDdc, on the GPU: the scene of
tests/test_fft_ddc_mixed_carriers.py made in one pass.  PacketTransmitter bursts at 4 samples per symbol, one row at
I = 4 on -0.31 and one at I = 16 on 0.17 (a quarter of the symbol rate), go through MixedFftDuc.pack(), process_bulk() and
flush(); noise is added; Spectrum().carriers() finds both carriers, fft_ddc_decimation() recovers the decimations 4 and 16
from the found bandwidths, MixedFftDdc(found frequencies, those decimations) brings the rows back, and a receiver per row
delivers every packet byte for byte.  The stream (before the noise) differs from the sum of _duc_ref.duc64 of each row
with the same taps by no more than the two bounds of tests/_fft_duc_mixed_ref.py together: the truncation to two images
and the first-order float32 bound of the device (measured on MI355X: 0.118 of them at most)."""
import numpy as np
import pytest

import _duc_ref as uref
import _fft_duc_mixed_ref as mref
import test_fft_ddc_mixed_carriers as scene26
from _frontend import host, load_package, received_packets

pytestmark = pytest.mark.gpu

CARRIERS, INTERPOLATIONS = scene26.CARRIERS, scene26.DECIMATIONS
ROW, WIDE = scene26.ROW, scene26.WIDE


def test_two_symbol_rates_from_one_handle_and_back():
    import torch
    pkg = load_package()
    sent, bursts = [], []
    for k in range(2):
        v, payloads = scene26.row_of_bursts(pkg, scene26.BURSTS[k], ROW[k], 2027 + k)
        bursts.append(v[0])
        sent.append(payloads)
    taps = [pkg.fft_duc_taps(I) for I in INTERPOLATIONS]
    up = pkg.MixedFftDuc(CARRIERS, INTERPOLATIONS)
    assert (up.overlap, up.hop, up.slot) == (mref.default_overlap_mixed(taps), mref.N - 256, 16)
    v, slots = up.pack(bursts)
    assert slots == ROW[1] and tuple(v.shape) == (2, ROW[0]) and list(up.items_for(slots)) == ROW
    body = up.process_bulk(v, slots)
    assert body.numel() == WIDE // up.hop * up.hop and up.pending == slots % (up.hop // 16)
    x = torch.cat([body, up.flush()]).contiguous()
    assert x.numel() % up.hop == 0 and x.numel() >= WIDE and up.pending == 0 and 200000 <= x.numel() <= 400000
    clean = x
    x = pkg.NoiseSource("gaussian", scene26.SIGMA, 5, "c64", max_items=x.numel()).process_bulk(x.numel(), add_to=x).contiguous()

    found = pkg.Spectrum().process_bulk(x).carriers()
    f = [float(c) for c in found["frequency"]]
    assert len(f) == 2, f
    D = [pkg.fft_ddc_decimation(float(w)) for w in found["bandwidth"]]
    print(f"found carriers {f} (set: {CARRIERS}), bandwidths {[float(w) for w in found['bandwidth']]} -> decimations {D}")
    assert D == INTERPOLATIONS
    down = pkg.MixedFftDdc(f, D)
    rows, lengths = down.process_bulk(x)
    for k in range(2):
        rx = pkg.NativePacketReceiver(max_items=int(lengths[k]), tags_cap=2048, syncword_threshold=20.0, decode_headers=True,
                                      packets_only=True)
        assert received_packets(rx.process_bulk(rows[k, :lengths[k]].contiguous())) == sent[k], k

    vs = [host(bursts[k]) for k in range(2)]
    got = host(clean)[:body.numel()].astype(np.complex128)
    duc = sum(uref.duc64(vs[k][None, :], taps[k], INTERPOLATIONS[k], [CARRIERS[k]], [1.0])[:got.size] for k in range(2))
    bound = np.repeat(mref.truncation_bound(vs, taps, INTERPOLATIONS, CARRIERS, None, up.overlap, 2), up.hop) + \
        mref.device_bound(vs, taps, INTERPOLATIONS, CARRIERS, None, up.overlap, 2)
    err = np.abs(got - duc)
    some = bound > 0  # a segment of silence on every row has the bound 0, and is 0
    print(f"MixedFftDuc against the sum of duc64: worst difference / bound {np.max(err[some] / bound[some]):.4f}, worst difference "
          f"{np.max(err):.3e} of {np.max(np.abs(duc)):.3f}")
    assert got.shape == bound.shape and np.all(err <= bound)
