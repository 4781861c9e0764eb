"""The loop of tests/test_fft_ddc_carriers.py with the FftDuc in the Duc's place, on the GPU: fast convolution at both ends.
test_spectrum_carriers.rows_of_bursts -> FftDuc(CARRIERS, 4, gains=GAINS) with its flush() + NoiseSource ->
Spectrum().carriers() -> FftDdc(found, 4) -> a receiver per row delivers every packet byte for byte; and the FftDuc's
samples differ from _duc_ref.duc64 of the same taps by no more than the two bounds of tests/_fft_duc_ref.py together: the
truncation to two images (Cauchy-Schwarz on the dropped bins) and the first-order float32 bound of the device."""
import numpy as np
import pytest

import _duc_ref as uref
import _fft_duc_ref as fref
import test_spectrum_carriers as scene5
from _frontend import host, load_package, received_packets

pytestmark = pytest.mark.gpu

I = 4
CARRIERS, GAINS, N = scene5.CARRIERS, scene5.GAINS, scene5.N


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def test_fft_duc_to_fft_ddc_to_packets(pkg):
    import torch
    v, sent = scene5.rows_of_bursts(pkg, len(CARRIERS), 2027)
    taps = pkg.fft_duc_taps(I)
    assert np.array_equal(taps, pkg.duc_taps(I))
    up = pkg.FftDuc(CARRIERS, I, gains=GAINS)
    V = fref.default_overlap(taps.size)
    assert (up.overlap, up.hop) == (V, fref.N - V)
    body = up.process_bulk(v)
    assert body.numel() == fref.segments(N, I, V) * up.hop and up.pending == N % (up.hop // I)
    x = torch.cat([body, up.flush()]).contiguous()
    assert x.numel() % up.hop == 0 and x.numel() >= (N - 1) * I + taps.size and up.pending == 0
    x = pkg.NoiseSource("gaussian", scene5.SIGMA, 5, "c64", max_items=x.numel()).process_bulk(x.numel(), add_to=x).contiguous()

    found = pkg.Spectrum().process_bulk(x).carriers()
    f = [float(c) for c in found["frequency"]]
    assert len(f) == len(CARRIERS), f
    assert all(scene5.distance(a, b) <= 0.00673 / I for a, b in zip(f, CARRIERS)), (f, CARRIERS)
    y = pkg.FftDdc(f, I).process_bulk(x)
    for k in range(len(CARRIERS)):
        rx = pkg.NativePacketReceiver(max_items=y.shape[1], tags_cap=2048, syncword_threshold=20.0, decode_headers=True,
                                      packets_only=True)
        assert received_packets(rx.process_bulk(y[k].contiguous())) == sent[k], k

    vs = host(v)
    got = host(body).astype(np.complex128)
    duc = uref.duc64(vs, taps, I, CARRIERS, GAINS)[:got.size]
    bound = np.repeat(fref.truncation_bound(vs, taps, I, CARRIERS, GAINS, V, 2), up.hop) + \
        fref.device_bound(vs, taps, I, CARRIERS, GAINS, V, 2)
    err = np.abs(got - duc)
    some = bound > 0  # a segment of silence on every row has the bound 0, and is 0
    print(f"FftDuc against duc64: worst difference / bound {np.max(err[some] / bound[some]):.4f}, worst difference {np.max(err):.3e} "
          f"of {np.max(np.abs(duc)):.3f}")
    assert np.all(err <= bound)
