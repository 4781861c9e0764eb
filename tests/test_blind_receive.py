"""The two loops the LineSpectrum block closes: a burst's carrier from the Spectrum's coarse estimate alone, and a
carrier's symbol rate from nothing.

(a) The scene of tests/test_extract_bursts.py, built again with the same constants: 3 carriers, 6 bursts each of 64-byte
    packets, I = 5, noise 0.05.  Spectrum().carriers()["frequency"] -- NOT the scene's CARRIERS -- tunes a first
    Ddc(found, 5); its burst rows go through LineSpectrum.carrier_offset, the median per carrier refines the frequency,
    and a second Ddc(found + offset / 5, 5) -> extract is received: one detector tag per row, every payload byte for byte.
    Every burst row's line has margin_db >= 6, and |refined - true| * 5 <= 1 / (4 * 2048) cycles per item, one bin of
    the fourth-power spectrum.
(b) One carrier at 25/4 wideband samples per receiver sample.  Spectrum finds it; at the provisional decimation
    floor(0.4 / bandwidth) its bursts are extracted, symbol_rate gives the rate, resample_ratio gives (4, 25), and
    Ddc([refined], 25, interpolation=4) -> NativePacketReceiver returns the four payloads.  The same through
    apps/packet_receiver_file.py --tune auto --refine --decimate auto on an sc16 file.

The parameters the specification leaves to the caller, and why.  hop = 256: a burst is 1936 items, shorter than a
segment; at hop 1024 two or three segments see it, each cut at another place of its window, at 256 a dozen placements
are averaged.  max_offset = 4 bins of the scan: find_carriers is good to one PSD bin, 1 / 2048 cycle per wideband sample,
that is D / 2048 cycles per item; four times that leaves room, and the fewer bins are searched, the fewer chances the
self-noise of x^4 (the items between the symbol instants of an unfiltered RRC burst) has to beat the line.

The CPU part holds the float64 restatement to the same two conditions (burst rows: margin_db >= 6 and the error bound;
a noise row: margin_db below every burst row's and below 6) on numpy bursts at Es/N0 = 20 dB, so that a failure on the GPU
is not one of the scene.  20 dB is a floor of the scene's, an estimate and not a measurement: the noise is at most
2 * 0.05^2 per wideband sample, of which the Ddc's low-pass keeps about a fifth, 0.001 per item; the weaker carrier
(gain 0.5) has about 0.06 per item, and Es/N0 = 4 * 0.06 / 0.001, about 24 dB."""
import importlib.util
import os

import numpy as np
import pytest

import _line_spectrum_ref as lref
from _frontend import load_package, received_packets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

I = 5
CARRIERS = [-0.37, 0.13, 0.41]
GAINS = [1.0, 0.5, 1.0]
BURSTS, PAYLOAD, GAP = 6, 64, 5000
FIRST_GAPS = [3000, 5200, 1100]
BURST = 4 * (4 * PAYLOAD + 228)
N = 50000
SIGMA = 0.05
HOP, R, FFT = 512, 4, 2048
ROW_SPAN = (R - 1) * HOP + FFT
N_COLS = 6144
LINE_HOP = 256
MIN_MARGIN_DB = 6.0
OFFSET_BOUND = 1.0 / (4 * FFT)  # cycles per item: one bin of the fourth-power spectrum


def scan_offset(D):
    """max_offset for rows at decimation D behind a scan: four PSD bins, in cycles per item"""
    return 4.0 * D / FFT


# ---- CPU: the restatement on synthetic bursts ----

def rrc(alpha=0.35, sps=4, span=11):
    t = np.arange(-(span * sps // 2), span * sps // 2 + 1) / sps
    h = np.empty_like(t)
    for i, u in enumerate(t):
        if u == 0:
            h[i] = 1 - alpha + 4 * alpha / np.pi
        else:
            h[i] = (np.sin(np.pi * u * (1 - alpha)) + 4 * alpha * u * np.cos(np.pi * u * (1 + alpha))) / (np.pi * u * (1 - (4 * alpha * u) ** 2))
    return h / np.sqrt(np.sum(h ** 2))


def synthetic_rows(seed, esn0_db=20.0, pad=700):
    """(burst row, its offset, noise row): 64 real +-1 symbols, then 420 diagonal QPSK symbols, RRC 0.35 at 4 samples per
    symbol with unit symbol energy, `pad` noise-only items on either side, complex noise of variance N0 per item"""
    rng = np.random.default_rng(seed)
    delta = rng.uniform(-1.0, 1.0) * I / FFT  # within one PSD bin of the scan
    sym = np.concatenate([rng.choice([-1.0, 1.0], 64).astype(complex),
                          (rng.choice([-1, 1], 420) + 1j * rng.choice([-1, 1], 420)) / np.sqrt(2)])
    up = np.zeros(sym.size * 4, complex)
    up[::4] = sym
    s = np.convolve(up, rrc())
    x = np.zeros(2 * pad + s.size, complex)
    x[pad:pad + s.size] = s
    x *= np.exp(2j * np.pi * delta * np.arange(x.size))
    n0 = 10.0 ** (-esn0_db / 10.0)
    noise = lambda: np.sqrt(n0 / 2) * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))
    return (x + noise()).astype(np.complex64), delta, noise().astype(np.complex64)


def ref_offset(row, max_offset):
    gain = 1.0 / np.sqrt(np.mean(np.abs(row.astype(np.complex128)) ** 2))
    sp = lref.row_spectrum(row, row.size, LINE_HOP, lref.hann(), "fourth", gain)["out"]
    half = int(np.floor(4 * max_offset * FFT))
    line = lref.find_line(sp, (FFT - half) % FFT, 2 * half + 1)
    return line["frequency"] / 4, line["margin_db"]


def test_the_restatement_keeps_both_conditions_on_synthetic_bursts():
    burst_margins, noise_margins, errors = [], [], []
    for seed in range(20):
        x, delta, noise = synthetic_rows(seed)
        f, m = ref_offset(x, scan_offset(I))
        burst_margins.append(m)
        errors.append(abs(f - delta))
        noise_margins.append(ref_offset(noise, scan_offset(I))[1])
    print(f"burst rows: margin_db {min(burst_margins):.2f} .. {max(burst_margins):.2f}, worst error {max(errors):.2e} "
          f"(bound {OFFSET_BOUND:.2e}); noise rows: margin_db up to {max(noise_margins):.2f}")
    assert min(burst_margins) >= MIN_MARGIN_DB
    assert max(errors) <= OFFSET_BOUND
    assert max(noise_margins) < min(min(burst_margins), MIN_MARGIN_DB)


# ---- GPU ----

@pytest.fixture(scope="module")
def pkg():
    return load_package()


def truth(k):
    return [(I * (FIRST_GAPS[k] + b * (BURST + GAP)), I * (FIRST_GAPS[k] + b * (BURST + GAP) + BURST)) for b in range(BURSTS)]


@pytest.fixture(scope="module")
def scene(pkg):
    """section 22's scene: the wideband stream [N I] on the device, the payloads per carrier, what a Spectrum finds"""
    import torch
    rng = np.random.default_rng(2028)
    tx = pkg.PacketTransmitter()
    v = torch.zeros((len(CARRIERS), N), dtype=torch.complex64, device="cuda")
    sent = []
    for k in range(len(CARRIERS)):
        payloads = [rng.integers(0, 256, PAYLOAD, dtype=np.uint8).tobytes() for _ in range(BURSTS)]
        tx.reset()
        b, offsets, lengths = tx.process_bulk(payloads, gaps=[FIRST_GAPS[k]] + [GAP] * (BURSTS - 1))
        assert [(I * int(o), I * int(o + n)) for o, n in zip(offsets, lengths)] == truth(k)
        v[k, :b.numel()] = b
        sent.append(payloads)
    x = pkg.Duc(CARRIERS, I, gains=GAINS).process_bulk(v)
    x = pkg.NoiseSource("gaussian", SIGMA, 5, "c64", max_items=N * I).process_bulk(N * I, add_to=x).contiguous()
    carriers = pkg.Spectrum().process_bulk(x).carriers()
    assert len(carriers) == len(CARRIERS)
    return x, sent, carriers


def packets_of_rows(pkg, rows, payloads):
    """(detector tags per row, rows whose one packet is its burst's payload): test_extract_bursts.py's receivers"""
    got = pkg.NativeMultiChannelReceiver(len(payloads), syncword_threshold=20.0, max_items=N_COLS).process_bulk(rows)
    tags = [int(got[r]["detector_tags"]["index"].size) for r in range(len(payloads))]
    good = []
    for r, payload in enumerate(payloads):
        rx = pkg.NativePacketReceiver(max_items=N_COLS, tags_cap=2048, packets_only=True, decode_headers=True, syncword_threshold=20.0)
        good.append(received_packets(rx.process_bulk(rows[r].contiguous())) == [payload])
    return tags, good


@pytest.mark.gpu
def test_carrier_offset_closes_the_loop_from_the_coarse_estimate(pkg, scene):
    x, sent, carriers = scene
    found = [float(c["frequency"]) for c in carriers]
    sg = pkg.Spectrogram(hop=HOP, average=R)
    power = sg.band_power(sg.process_bulk(x), carriers)
    bursts = [sg.bursts(power[k]) for k in range(len(CARRIERS))]
    assert [len(b) for b in bursts] == [BURSTS] * len(CARRIERS)
    margin = -(-ROW_SPAN // I)
    payloads = [p for k in range(len(CARRIERS)) for p in sent[k]]

    def rows_of(frequencies, extra=()):
        d = pkg.Ddc(frequencies, I)
        spans = [s for k in range(len(CARRIERS)) for s in d.burst_spans(bursts[k], k, margin_frames=margin)] + list(extra)
        return d.extract(x, spans, n_cols=N_COLS)

    # the first pass on the coarse frequencies; row 18 is carrier 0's silence in front of its first burst
    rows, lengths = rows_of(found, extra=[(0, 0, FIRST_GAPS[0] - 400)])
    ls = pkg.LineSpectrum(hop=LINE_HOP)
    lines = ls.carrier_offset(rows, lengths, max_offset=scan_offset(I))
    burst_lines, noise_line = lines[:18], lines[18]
    refined = [found[k] + float(np.median(burst_lines["offset"][k * BURSTS:(k + 1) * BURSTS])) / I for k in range(len(CARRIERS))]
    coarse_err = [abs(f - t) * I for f, t in zip(found, CARRIERS)]
    refined_err = [abs(f - t) * I for f, t in zip(refined, CARRIERS)]
    print("margin_db per burst row:", np.round(burst_lines["margin_db"], 2).tolist(), " noise row:", round(float(noise_line["margin_db"]), 2))
    print("coarse errors (cycles per item):", coarse_err, " refined:", refined_err, " bound:", OFFSET_BOUND)
    tags, good = packets_of_rows(pkg, rows[:18], payloads)
    print(f"the coarse frequencies alone: {sum(good)} of 18 packets, detector tags per row {tags} (reported, not asserted)")

    assert np.all(burst_lines["margin_db"] >= MIN_MARGIN_DB)
    assert noise_line["margin_db"] < min(float(burst_lines["margin_db"].min()), MIN_MARGIN_DB)
    assert all(e <= OFFSET_BOUND for e in refined_err)

    rows2, _ = rows_of(refined)
    tags, good = packets_of_rows(pkg, rows2, payloads)
    assert tags == [1] * 18, f"detector tags per row {tags}"
    assert all(good), good


# scene (b): 4 bursts at 25/4 wideband samples per receiver sample
B_CARRIER, B_BURSTS, B_GAP, B_TAIL = 0.13, 4, 5000, 4000


@pytest.fixture(scope="module")
def scene_b(pkg):
    import torch
    rng = np.random.default_rng(2029)
    payloads = [rng.integers(0, 256, PAYLOAD, dtype=np.uint8).tobytes() for _ in range(B_BURSTS)]
    b, _, _ = pkg.PacketTransmitter().process_bulk(payloads, gaps=[3000] + [B_GAP] * (B_BURSTS - 1))
    v = torch.cat([b, torch.zeros(B_TAIL, dtype=torch.complex64, device="cuda")])[None, :].contiguous()
    x = pkg.Duc([B_CARRIER], 25, decimation=4, max_items=v.shape[1]).process_bulk(v).contiguous()
    x = pkg.NoiseSource("gaussian", SIGMA, 7, "c64", max_items=x.numel()).process_bulk(x.numel(), add_to=x).contiguous()
    return x, payloads


def blind_parameters(pkg, x):
    """(refined frequency, (I, D), D0, the lines) of the one carrier in x, from nothing"""
    carriers = pkg.Spectrum().process_bulk(x).carriers()
    assert len(carriers) == 1
    f0, d0 = float(carriers[0]["frequency"]), pkg.provisional_decimation(float(carriers[0]["bandwidth"]))
    sg = pkg.Spectrogram(hop=HOP, average=R)
    found = sg.bursts(sg.band_power(sg.process_bulk(x), carriers)[0])
    assert len(found) == B_BURSTS
    d = pkg.Ddc([f0], d0)
    rows, lengths = d.extract(x, d.burst_spans(found, 0, margin_frames=-(-ROW_SPAN // d0)))
    ls = pkg.LineSpectrum(hop=LINE_HOP)
    rates = ls.symbol_rate(rows, lengths)
    offsets = ls.carrier_offset(rows, lengths, max_offset=scan_offset(d0))
    ratio = pkg.resample_ratio(float(np.median(rates["rate"])) / d0)
    return f0 + float(np.median(offsets["offset"])) / d0, ratio, d0, rates, offsets, f0


@pytest.mark.gpu
def test_symbol_rate_closes_the_loop_from_nothing(pkg, scene_b):
    x, payloads = scene_b
    refined, ratio, d0, rates, offsets, f0 = blind_parameters(pkg, x)
    print(f"provisional decimation {d0}; rate per item {rates['rate'].tolist()} (true {0.04 * d0}), margin_db "
          f"{np.round(rates['margin_db'], 2).tolist()}; carrier found {f0:+.6f} refined {refined:+.7f} (true {B_CARRIER}), "
          f"offset margin_db {np.round(offsets['margin_db'], 2).tolist()}")
    assert ratio == (4, 25)
    assert np.all(offsets["margin_db"] >= MIN_MARGIN_DB)
    assert np.all(np.abs(rates["rate"] / d0 / 0.04 - 1.0) <= 2e-4)  # resample_ratio's rel_tol of 2e-3 rests on this figure
    y = pkg.Ddc([refined], 25, interpolation=4).process_bulk(x)
    rx = pkg.NativePacketReceiver(max_items=y.shape[1], tags_cap=2048, syncword_threshold=20.0, decode_headers=True, packets_only=True)
    assert received_packets(rx.process_bulk(y[0].contiguous())) == payloads


def load_app(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "apps", name + ".py"))
    app = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(app)
    return app


@pytest.mark.gpu
def test_the_file_app_receives_blind(pkg, scene_b, tmp_path, capsys):
    """scene (b) as an sc16 file -> packet_receiver_file.py --tune auto --refine --decimate auto: the packets"""
    x, payloads = scene_b
    path, out = str(tmp_path / "wideband.sc16"), str(tmp_path / "packets.bin")
    xr = np.ascontiguousarray(x.cpu().numpy()).view(np.float32).reshape(-1, 2)
    assert np.abs(xr).max() * 4096.0 < 32767
    np.round(xr * 4096.0).astype("<i2").tofile(path)
    app = load_app("packet_receiver_file")
    app.main([path, "4", "20.0", "--format", "sc16", "--scale", str(1.0 / 4096.0), "--tune", "auto", "--refine",
              "--decimate", "auto", "--chunk-items", "200000", "--out", out])
    text = capsys.readouterr().out
    print(text)
    assert "--decimate auto:" in text and "--decimate 25/4" in text and "--refine:" in text
    got, data, pos = [], open(out, "rb").read(), 0
    while pos < len(data):
        n = int.from_bytes(data[pos:pos + 2], "big")
        got.append(data[pos + 2:pos + 2 + n])
        pos += 2 + n
    assert got == payloads
