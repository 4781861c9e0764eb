"""The loop of tests/test_spectrum_carriers.py with the FftDdc in the Ddc's place, on the GPU: its scene with Duc(..., 4)
instead of 5; Spectrum().process_bulk(x).carriers() -> FftDdc(found["frequency"], 4) -> a receiver per row delivers every
packet byte for byte; and the rows differ from Ddc(found["frequency"], 4, taps=the same) by no more than the two bounds
of tests/_fft_ddc_ref.py together: the truncation to two images (Cauchy-Schwarz on the dropped bins) and the first-order
float32 bound of the device."""
import numpy as np
import pytest

import _fft_ddc_ref as fref
import test_spectrum_carriers as scene5
from _frontend import host, load_package, received_packets

pytestmark = pytest.mark.gpu

D = 4
CARRIERS, GAINS, N = scene5.CARRIERS, scene5.GAINS, scene5.N


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def test_found_carriers_through_the_fft_ddc(pkg):
    v, sent = scene5.rows_of_bursts(pkg, len(CARRIERS), 2027)
    x = pkg.Duc(CARRIERS, D, gains=GAINS).process_bulk(v)
    x = pkg.NoiseSource("gaussian", scene5.SIGMA, 5, "c64", max_items=N * D).process_bulk(N * D, add_to=x).contiguous()
    found = pkg.Spectrum().process_bulk(x).carriers()
    f = [float(c) for c in found["frequency"]]
    # three carriers, each inside the detector's pull-in of 0.00673 / D cycles per wideband sample (3.4 PSD bins at D = 4;
    # the carriers are 5 / 4 as wide as in the scene at 5, and the scan resolves a bin)
    assert len(f) == len(CARRIERS), f
    assert all(scene5.distance(a, b) <= 0.00673 / D for a, b in zip(f, CARRIERS)), (f, CARRIERS)
    taps = pkg.fft_ddc_taps(D)
    assert np.array_equal(taps, pkg.ddc_taps(D))
    b = pkg.FftDdc(f, D)
    assert (b.overlap, b.hop) == (fref.default_overlap(taps.size), fref.N - fref.default_overlap(taps.size))
    y = b.process_bulk(x)
    frames = fref.segments(N * D, D, b.overlap) * b.hop // D
    assert tuple(y.shape) == (len(CARRIERS), frames) and N - frames <= b.hop // D
    for k in range(len(CARRIERS)):
        rx = pkg.NativePacketReceiver(max_items=N, tags_cap=2048, syncword_threshold=20.0, decode_headers=True, packets_only=True)
        assert received_packets(rx.process_bulk(y[k].contiguous())) == sent[k], k

    ddc = host(pkg.Ddc(f, D, taps=taps).process_bulk(x))[:, :frames]
    xs = host(x)
    bound = np.repeat(fref.truncation_bound(xs, taps, D, f, b.overlap, 2), b.hop // D, axis=1) + fref.device_bound(xs, taps, D, f, b.overlap, 2)
    err = np.abs(host(y).astype(np.complex128) - ddc.astype(np.complex128))
    print(f"FftDdc against Ddc: worst difference / bound {np.max(err / bound):.4f}, worst difference {np.max(err):.3e} "
          f"of {np.max(np.abs(ddc)):.3f}")
    assert np.all(err <= bound)
