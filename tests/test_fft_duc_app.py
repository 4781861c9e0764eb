"""apps/packet_transmitter_file.py --fft-duc --tune 0.13 --interpolate 4 (its function, in process): three 64-byte packets
become a wideband file through the FftDuc and its flush(); apps/packet_receiver_file.py --tune 0.13 --decimate 4 returns
them, and so does its --fft-ddc.  Without a carrier offset and an integer interpolation the option is refused."""
import importlib.util
import os

import numpy as np
import pytest

from _frontend import load_package

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def load_app(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "apps", name + ".py"))
    app = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(app)
    return app


def test_three_packets_through_the_file_apps(pkg, tmp_path):
    txa, rxa = load_app("packet_transmitter_file"), load_app("packet_receiver_file")
    rng = np.random.default_rng(2028)
    sent = [rng.integers(0, 256, 64, dtype=np.uint8).tobytes() for _ in range(3)]
    path = str(tmp_path / "wideband.cf32")
    for bad in (dict(tune=0.13), dict(interpolate=4), dict(tune=0.13, interpolate="25/4")):
        with pytest.raises(ValueError):
            txa.transmit(sent, path, gap=3000, pkg=pkg, fft_duc=True, **bad)
    with pytest.raises(pkg.Gr4pmError):
        txa.transmit(sent, path, gap=3000, pkg=pkg, fft_duc=True, tune=0.13, interpolate=5)
    written = txa.transmit(sent, path, gap=3000, pkg=pkg, fft_duc=True, tune=0.13, interpolate=4)
    # whole segments of the default shape at I = 4 (48 taps, an overlap of 256, a hop of 1792), and all of every burst
    items = sum(3000 + 4 * (4 * len(p) + 228) for p in sent)
    assert os.path.getsize(path) == 8 * written and written % 1792 == 0 and 4 * (items - 1) + 48 <= written < 4 * items + 48 + 1792
    with open(path, "ab") as f:  # silence behind the last burst, as in front of every other one
        f.write(np.zeros(8192 * 4, dtype=np.complex64).tobytes())
    r = rxa.receive_file(path, syncword_threshold=20.0, chunk_items=50000, pkg=pkg, tune=0.13, decimate=4)
    assert r["packets"] == sent
    r = rxa.receive_file(path, syncword_threshold=20.0, chunk_items=50000, pkg=pkg, tune=0.13, decimate=4, fft_ddc=True)
    assert r["packets"] == sent
