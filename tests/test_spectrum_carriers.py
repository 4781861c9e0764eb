"""The loop the Spectrum block closes, on the GPU: PacketTransmitter bursts on three carriers -> Duc -> NoiseSource make a
wideband stream; Spectrum().process_bulk(x).carriers() finds exactly the three carriers within one PSD bin (1 / 2048
cycles per sample) of their centres -- the detector's pull-in at a decimation of 5 is 0.00673 / 5 = 2.76 bins --; a Ddc
tuned to the FOUND centres feeds receivers that deliver every packet; a carrier across +-0.5 is one carrier; and
apps/packet_receiver_file.py --scan prints the same three frequencies for an sc16 file of the stream."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _spectrum_ref as sref
from _frontend import load_package, received_packets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I = 5
CARRIERS = [-0.37, 0.13, 0.41]
GAINS = [1.0, 0.5, 1.0]
BURSTS, PAYLOAD, GAP = 12, 64, 600
BURST = 4 * (4 * PAYLOAD + 228)  # items of one shaped burst at 4 samples per symbol
N = BURSTS * (BURST + GAP) + 9500  # items per row; the receiver delivers a packet once the stream goes on well behind it
BIN = 1.0 / 2048
SIGMA = 0.05


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def rows_of_bursts(pkg, K, seed):
    """[K, N] rows of BURSTS bursts each, and the payloads"""
    import torch
    rng = np.random.default_rng(seed)
    tx = pkg.PacketTransmitter()
    v = torch.zeros((K, N), dtype=torch.complex64, device="cuda")
    sent = []
    for k in range(K):
        payloads = [rng.integers(0, 256, PAYLOAD, dtype=np.uint8).tobytes() for _ in range(BURSTS)]
        tx.reset()
        b, _, _ = tx.process_bulk(payloads, gaps=[GAP] * BURSTS)
        assert b.numel() == BURSTS * (BURST + GAP) <= N
        v[k, :b.numel()] = b
        sent.append(payloads)
    return v, sent


def wideband(pkg, v, carriers, gains, seed=5):
    x = pkg.Duc(carriers, I, gains=gains).process_bulk(v)
    return pkg.NoiseSource("gaussian", SIGMA, seed, "c64", max_items=N * I).process_bulk(N * I, add_to=x)


@pytest.fixture(scope="module")
def scene(pkg):
    v, sent = rows_of_bursts(pkg, len(CARRIERS), 2027)
    x = wideband(pkg, v, CARRIERS, GAINS).contiguous()
    return x, sent


def distance(f, g):
    """on the circle of frequencies"""
    d = abs(f - g) % 1.0
    return min(d, 1.0 - d)


def assert_the_three(freqs):
    assert len(freqs) == len(CARRIERS), freqs
    for f, want in zip(freqs, CARRIERS):
        assert distance(float(f), want) <= BIN, (freqs, CARRIERS)


def test_every_carrier_is_inside_a_hundred_segments():
    """burst b of a row covers the wideband samples [I (b (BURST + GAP) + GAP), + I BURST); segment s the samples
    [1024 s, 1024 s + 2048)"""
    S = sref.segments(N * I, 1024)
    inside = 0
    for s in range(S):
        lo, hi = 1024 * s, 1024 * s + 2048
        inside += any(lo < I * (b * (BURST + GAP) + GAP) + I * BURST and I * (b * (BURST + GAP) + GAP) < hi for b in range(BURSTS))
    assert inside >= 100, inside


def test_found_centres(pkg, scene):
    x, _ = scene
    # the float64 reference on the same samples meets both conditions: three carriers, each within a bin
    ref = sref.welch(x.cpu().numpy(), 1024, sref.hann())
    want = sref.find_carriers(ref["max_hold"])
    print("float64 reference:", [(round(c["frequency"], 6), c["n_bins"], round(c["snr_db"], 1)) for c in want])
    assert_the_three([c["frequency"] for c in want])
    sp = pkg.Spectrum().process_bulk(x)
    got = sp.carriers()
    print("found:", [(round(float(c["frequency"]), 6), int(c["n_bins"]), round(float(c["snr_db"]), 1)) for c in got])
    assert sp.read()["segments"] == ref["segments"] >= 100
    assert_the_three(got["frequency"])
    # the carrier at half the amplitude has a quarter of the power: the strongest is not that one
    assert int(np.argmax(got["power"])) != 1
    # the mean spectrum of a stream that is mostly bursts finds them too
    assert_the_three(sp.carriers(which="mean")["frequency"])


@pytest.mark.parametrize("centres", ["found", "true"])
def test_receive_at_the_centres(pkg, scene, centres):
    x, sent = scene
    f = [float(c) for c in pkg.Spectrum().process_bulk(x).carriers()["frequency"]] if centres == "found" else CARRIERS
    assert len(f) == len(CARRIERS)
    y = pkg.Ddc(f, I).process_bulk(x)
    assert tuple(y.shape) == (len(CARRIERS), N)
    for k in range(len(CARRIERS)):
        rx = pkg.NativePacketReceiver(max_items=N, tags_cap=2048, syncword_threshold=20.0, decode_headers=True, packets_only=True)
        assert received_packets(rx.process_bulk(y[k].contiguous())) == sent[k], k


def test_a_carrier_across_the_wrap_is_one(pkg):
    v, _ = rows_of_bursts(pkg, 1, 7)
    x = wideband(pkg, v, [0.499], None)
    got = pkg.Spectrum().process_bulk(x).carriers()
    assert len(got) == 1, got
    assert distance(float(got[0]["frequency"]), 0.499) <= BIN
    assert -0.5 <= got[0]["frequency"] < 0.5
    assert int(got[0]["first_bin"]) < 1024 <= int(got[0]["first_bin"]) + int(got[0]["n_bins"])  # it spans bin 1024


def test_app_scan(pkg, scene, tmp_path):
    x, _ = scene
    path = str(tmp_path / "wideband.sc16")
    pkg.iq_pack(x, "sc16", gain=8192.0).cpu().numpy().tofile(path)
    assert os.path.getsize(path) == 4 * N * I and N * I <= 1 << 20
    r = subprocess.run([sys.executable, os.path.join(ROOT, "apps", "packet_receiver_file.py"), path, "--format", "sc16", "--scan"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = re.findall(r"^carrier frequency (\S+) bandwidth (\S+) snr_db (\S+)$", r.stdout, flags=re.M)
    assert_the_three([float(f) for f, _, _ in lines])
    assert "packets" not in r.stdout  # it exits after the scan
