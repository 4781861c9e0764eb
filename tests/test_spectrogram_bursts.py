"""The loop the Spectrogram block closes, on the GPU: PacketTransmitter bursts on three carriers, NOT aligned in time ->
Duc -> NoiseSource make a wideband stream; Spectrum().process_bulk(x).carriers() finds the carriers,
Spectrogram.band_power() the power of each carrier's band per row, Spectrogram.bursts() the six bursts of each carrier
with their first and last sample within one row's span of the truth; and apps/packet_receiver_file.py --scan --bursts
prints the same for an sc16 file of the stream.

The scene is the one of tests/test_spectrum_carriers.py with 6 bursts per row, gaps of 5000 items and a different first
gap per row, so a wrong band gives wrong times."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _spectrogram_ref as gref
import _spectrum_ref as sref
from _frontend import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I = 5
CARRIERS = [-0.37, 0.13, 0.41]
GAINS = [1.0, 0.5, 1.0]
BURSTS, PAYLOAD, GAP = 6, 64, 5000
FIRST_GAPS = [3000, 5200, 1100]
BURST = 4 * (4 * PAYLOAD + 228)  # items of one shaped burst at 4 samples per symbol
N = 50000  # items per row: the last burst ends at 5200 + 6 * 1936 + 5 * 5000 = 41816
SIGMA = 0.05
SHAPES = [(512, 1), (512, 4), (1024, 2)]  # (hop, R)
FFT = 2048


def truth(k):
    """[(a, e)]: burst b of row k covers the wideband samples [a, e)"""
    return [(I * (FIRST_GAPS[k] + b * (BURST + GAP)), I * (FIRST_GAPS[k] + b * (BURST + GAP) + BURST)) for b in range(BURSTS)]


def test_the_scene_keeps_the_median_a_noise_row():
    """from the known offsets alone, at every (hop, R) used: the rows that touch a burst of a carrier are fewer than 40 %
    of all rows, so the lower median of its band's power is a noise row; every gap between two bursts leaves at least 3
    rows clear of any burst, so no two bursts merge; and the three rows' bursts are not aligned in time"""
    assert max(FIRST_GAPS) + BURSTS * BURST + (BURSTS - 1) * GAP <= N
    for hop, R in SHAPES:
        adv, span = R * hop, (R - 1) * hop + FFT
        rows = gref.n_rows(N * I, hop, R)
        lo, hi = np.arange(rows) * adv, np.arange(rows) * adv + span
        for k in range(len(CARRIERS)):
            touch = np.zeros(rows, dtype=bool)
            for a, e in truth(k):
                touch |= (lo < e) & (a < hi)
            assert touch.sum() < 0.4 * rows, (hop, R, k, int(touch.sum()), rows)
            t = truth(k)
            for (_, e), (a, _) in zip(t[:-1], t[1:]):
                assert np.sum((lo >= e) & (hi <= a)) >= 3, (hop, R, k)
    starts = sorted(a for k in range(len(CARRIERS)) for a, _ in truth(k))
    assert min(np.diff(starts)) >= 1000 * I


def assert_the_bursts(found, k, span, what):
    """exactly 6 bursts; the b-th starts and ends within one row's span of the truth"""
    t = truth(k)
    got = [(int(b["start_sample"]), int(b["end_sample"])) for b in found] if not isinstance(found, list) else found
    assert len(got) == BURSTS, f"{what}: carrier {k}: {len(got)} bursts, not {BURSTS}: {got}"
    for (s, e), (a, end) in zip(got, t):
        assert abs(s - a) < span and abs(e - end) < span, f"{what}: carrier {k}: [{s}, {e}) against [{a}, {end}), span {span}"


# ---- GPU ----

@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def scene(pkg):
    """the wideband stream [N I] on the device, and the carriers a Spectrum finds in it"""
    import torch
    rng = np.random.default_rng(2028)
    tx = pkg.PacketTransmitter()
    v = torch.zeros((len(CARRIERS), N), dtype=torch.complex64, device="cuda")
    for k in range(len(CARRIERS)):
        payloads = [rng.integers(0, 256, PAYLOAD, dtype=np.uint8).tobytes() for _ in range(BURSTS)]
        tx.reset()
        b, offsets, lengths = tx.process_bulk(payloads, gaps=[FIRST_GAPS[k]] + [GAP] * (BURSTS - 1))
        assert [(I * int(o), I * int(o + n)) for o, n in zip(offsets, lengths)] == truth(k)  # the transmitter's offset and length x 5
        v[k, :b.numel()] = b
    x = pkg.Duc(CARRIERS, I, gains=GAINS).process_bulk(v)
    x = pkg.NoiseSource("gaussian", SIGMA, 5, "c64", max_items=N * I).process_bulk(N * I, add_to=x).contiguous()
    sp = pkg.Spectrum().process_bulk(x)
    carriers = sp.carriers()
    assert len(carriers) == len(CARRIERS) and all(abs(float(c["frequency"]) - f) <= 1.0 / FFT for c, f in zip(carriers, CARRIERS))
    return x, carriers, sp.read()["mean"]


@pytest.mark.gpu
@pytest.mark.parametrize("hop,R", SHAPES)
def test_bursts_of_every_carrier(pkg, scene, hop, R):
    x, carriers, _ = scene
    bands = [(int(c["first_bin"]), int(c["n_bins"])) for c in carriers]
    sg = pkg.Spectrogram(hop=hop, average=R)
    assert (sg.row_advance, sg.row_span) == (R * hop, (R - 1) * hop + FFT)
    # the float64 restatement on the same samples meets the criterion: the scene is good
    rows64 = gref.rows(x.cpu().numpy(), hop, R, "mean", sref.hann())
    power64 = gref.band_power(rows64, bands)
    for k in range(len(CARRIERS)):
        assert_the_bursts(gref.spans(gref.find_bursts(power64[k]), sg.row_advance, sg.row_span), k, sg.row_span, "float64 restatement")
    rows = sg.process_bulk(x)
    assert tuple(rows.shape) == rows64.shape
    power = sg.band_power(rows, carriers)
    assert tuple(power.shape) == (len(CARRIERS), rows.shape[0])
    for k in range(len(CARRIERS)):
        found = sg.bursts(power[k])
        print(f"hop {hop} R {R} carrier {k}:", [(int(b["start_sample"]), int(b["end_sample"]), round(float(b["snr_db"]), 1)) for b in found])
        assert_the_bursts(found, k, sg.row_span, "Spectrogram")
        assert np.all(found["peak_row"] >= found["first_row"]) and np.all(found["peak_row"] < found["first_row"] + found["n_rows"])


@pytest.mark.gpu
def test_an_explicit_floor_finds_the_same_bursts(pkg, scene):
    """floor = the band's bins x the lower median of the Spectrum's mean (a noise bin: the carriers fill a fifth of them)"""
    x, carriers, mean = scene
    sg = pkg.Spectrogram(hop=512, average=4)
    power = sg.band_power(sg.process_bulk(x), carriers)
    noise_bin = float(np.sort(mean)[(mean.size - 1) // 2])
    for k, c in enumerate(carriers):
        by_floor = sg.bursts(power[k], floor=int(c["n_bins"]) * noise_bin)
        assert_the_bursts(by_floor, k, sg.row_span, "explicit floor")
        assert np.array_equal(by_floor["peak_row"], sg.bursts(power[k])["peak_row"])  # the floor does not move a maximum
    # rows handed over in two parts: first_row places the second part's bursts in the stream
    half = power.shape[1] // 2
    late = sg.bursts(power[0, half:], first_row=half, floor=int(carriers[0]["n_bins"]) * noise_bin)
    every = sg.bursts(power[0], floor=int(carriers[0]["n_bins"]) * noise_bin)
    assert len(late) >= 2 and np.array_equal(late["end_sample"][-2:], every["end_sample"][-2:])


@pytest.mark.gpu
def test_app_scan_bursts_and_waterfall(pkg, scene, tmp_path):
    x, _, _ = scene
    path, npy = str(tmp_path / "wideband.sc16"), str(tmp_path / "rows.npy")
    pkg.iq_pack(x, "sc16", gain=8192.0).cpu().numpy().tofile(path)
    assert os.path.getsize(path) == 4 * N * I and N * I <= 1 << 20
    app = [sys.executable, os.path.join(ROOT, "apps", "packet_receiver_file.py"), path, "--format", "sc16", "--scan"]
    r = subprocess.run(app + ["--bursts", "--waterfall", npy, "--waterfall-average", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    carriers = re.findall(r"^carrier frequency (\S+) bandwidth (\S+) snr_db (\S+)$", r.stdout, flags=re.M)
    assert len(carriers) == len(CARRIERS) and all(abs(float(c[0]) - f) <= 1.0 / FFT for c, f in zip(carriers, CARRIERS))
    lines = re.findall(r"^burst frequency (\S+) start (\d+) end (\d+) snr_db (\S+)$", r.stdout, flags=re.M)
    assert len(lines) == len(CARRIERS) * BURSTS, r.stdout
    span = 1024 + FFT  # hop 1024, R = 2
    for k, c in enumerate(carriers):
        assert_the_bursts([(int(s), int(e)) for f, s, e, _ in lines if f == c[0]], k, span, "app")
    assert r.stdout.index("burst frequency") > r.stdout.rindex("carrier frequency")  # after the carrier lines
    assert "packets" not in r.stdout  # it exits after the scan
    rows = np.load(npy)
    assert rows.dtype == np.float32 and rows.shape == (gref.n_rows(N * I, 1024, 2), FFT)
