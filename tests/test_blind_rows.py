"""The burst chain to the end: Spectrum -> Spectrogram bursts -> Ddc.extract at the provisional
decimation -> LineSpectrum per-row rate and offset -> RowResampler.to_samples_per_symbol -> the receivers.  No
resample_ratio, no second Ddc, the wideband stream is read once.

(a) tests/test_blind_receive.py's scene (b): one carrier at 25/4 wideband samples per receiver sample, 4 bursts, noise 0.05.
    One detector tag per row, every payload byte for byte.
(b) The same carrier plus one at 24.69 wideband samples per symbol (PfbArbResampler(1.2345) -> Duc(5)), summed: a rate that
    is no simple fraction of the recording's.  Both carriers' rows go through ONE RowResampler call with per-row steps and
    words; every payload of both is returned.  What resample_ratio makes of the second carrier is printed.
(c) (a) through apps/packet_receiver_file.py --burst-rows --tune auto --refine --decimate auto on an sc16 file.

Row parameters: a row whose carrier line has margin_db < 6 takes its carrier's medians; a row whose envelope line has
margin_db < 6 takes the carrier's median rate over the rows that pass both (section 23's second limit).

The CPU part states first what the definition makes of such a burst, in float64: a noiseless QPSK RRC burst at 0.28 symbols
per item with an offset of 0.003, resampled with the rate off by section 23's 3e-5.  Two figures, each held to a bound that
comes from the scene and not from the code:
  * against the same burst evaluated at the output instants: at most -40 dB.  The loop scenes have about 18 dB of signal
    to noise per row item (noise 0.001 per item against 0.06, tests/test_blind_receive.py), so -40 dB is 22 dB below it.
  * against the ideal 4-samples-per-symbol grid: the rate error moves the last of 484 symbols by 3e-5 * 484 = 0.0145
    symbols; a timing error of tau symbols changes a signal of at most (1 + 0.35) / 2 cycles per symbol by at most
    2 pi 0.675 tau / 2 of its size at rms frequency, 0.031 at the burst's end, that is -30 dB; the rms over the burst is
    held to that."""
import numpy as np
import pytest

import _row_resampler_ref as ref
from _frontend import load_package, received_packets
from test_blind_receive import (B_BURSTS, B_CARRIER, B_GAP, B_TAIL, HOP, LINE_HOP, MIN_MARGIN_DB, N_COLS, PAYLOAD, R, ROW_SPAN,
                                load_app, scan_offset, scene_b)  # noqa: F401  (scene_b is a fixture)

TWO32 = 1 << 32
ROW_COLS = 4096  # of the extracted rows: a burst with its margins is about 3100 items at the provisional decimation


# ---- CPU: what the definition makes of a burst ----

def rrc_pulse(t, alpha=0.35, span=11):
    """the root-raised-cosine pulse at t symbols, cut at +- span / 2"""
    t = np.asarray(t, dtype=np.float64)
    out = np.zeros_like(t)
    live = np.abs(t) <= span / 2
    u = t[live]
    with np.errstate(divide="ignore", invalid="ignore"):
        p = (np.sin(np.pi * u * (1 - alpha)) + 4 * alpha * u * np.cos(np.pi * u * (1 + alpha))) / (np.pi * u * (1 - (4 * alpha * u) ** 2))
    p[u == 0] = 1 - alpha + 4 * alpha / np.pi
    edge = np.isclose(np.abs(u), 1 / (4 * alpha))
    p[edge] = alpha / np.sqrt(2) * ((1 + 2 / np.pi) * np.sin(np.pi / (4 * alpha)) + (1 - 2 / np.pi) * np.cos(np.pi / (4 * alpha)))
    out[live] = p
    return out


def burst_at(t, symbols):
    """s(t) = sum_k a_k p(t - k), t in symbols"""
    t = np.asarray(t, dtype=np.float64)
    out = np.zeros(t.size, dtype=np.complex128)
    for lo in range(0, t.size, 512):
        tt = t[lo:lo + 512]
        out[lo:lo + 512] = rrc_pulse(tt[:, None] - np.arange(symbols.size)[None, :]) @ symbols
    return out


def test_what_the_definition_makes_of_a_burst():
    pkg_taps = ref.kaiser_taps64(32, 12).astype(np.float32)
    Q, P = 32, 12
    rng = np.random.default_rng(31)
    sym = (rng.choice([-1, 1], 484) + 1j * rng.choice([-1, 1], 484)) / np.sqrt(2)
    rho, delta, t0 = 0.28, 0.003, -8.0  # symbols per item, cycles per item, the first item's time in symbols
    n = int((484 + 16) / rho)
    i = np.arange(n)
    x = burst_at(i * rho + t0, sym) * np.exp(2j * np.pi * delta * i)
    delay = (Q * P - 1) / (2 * Q)
    for rate_error in (0.0, 3e-5):
        step = round(TWO32 / (4 * rho * (1 + rate_error)))
        freq = round(delta * TWO32)
        y = ref.resample64(x, n, pkg_taps, Q, step, 0, freq)
        pos = np.arange(y.size) * (step / TWO32)
        live = (pos > 2 * P) & (pos < n - 2 * P)  # the burst, not the filter's run-in and run-out
        turn = np.exp(-2j * np.pi * delta * delay)  # the mixer turns by the position, the filter delays by `delay`
        direct = burst_at((pos - delay) * rho + t0, sym) * turn
        scale = np.sqrt(np.mean(np.abs(direct[live]) ** 2))
        at_instants = 20 * np.log10(np.sqrt(np.mean(np.abs(y[live] - direct[live]) ** 2)) / scale)
        ideal = burst_at((np.arange(y.size) / 4.0 - delay * rho) + t0, sym) * turn  # 4 samples per symbol from the same start
        on_grid = 20 * np.log10(np.sqrt(np.mean(np.abs(y[live] - ideal[live]) ** 2)) / scale)
        drift = abs(pos[live][-1] * rho - np.arange(y.size)[live][-1] / 4.0)
        print(f"rate off by {rate_error:g}: error at the output instants {at_instants:.1f} dB, against the 4-per-symbol grid "
              f"{on_grid:.1f} dB (the last symbol is {drift:.4f} symbols off)")
        assert at_instants <= -40.0
        assert on_grid <= -30.0
        assert drift <= 3e-5 * 500 + 1e-4


# ---- GPU ----

@pytest.fixture(scope="module")
def pkg():
    return load_package()


def burst_rows(pkg, x, carrier):
    """(rows [B, ROW_COLS], lengths, per-row rate in symbols per item, per-row offset in cycles per item, D0) of one
    carrier of find_carriers: its bursts at the provisional decimation and what the LineSpectrum reads from them"""
    f0, d0 = float(carrier["frequency"]), pkg.provisional_decimation(float(carrier["bandwidth"]))
    sg = pkg.Spectrogram(hop=HOP, average=R)
    found = sg.bursts(sg.band_power(sg.process_bulk(x), np.array([carrier], dtype=carrier.dtype))[0])
    d = pkg.Ddc([f0], d0)
    rows, lengths = d.extract(x, d.burst_spans(found, 0, margin_frames=-(-ROW_SPAN // d0)), n_cols=ROW_COLS)
    ls = pkg.LineSpectrum(hop=LINE_HOP)
    rates = ls.symbol_rate(rows, lengths)
    offsets = ls.carrier_offset(rows, lengths, max_offset=scan_offset(d0))
    good = offsets["margin_db"] >= MIN_MARGIN_DB
    assert good.any(), offsets
    timed = good & (rates["margin_db"] >= MIN_MARGIN_DB)
    rate, offset = rates["rate"].copy(), offsets["offset"].copy()
    offset[~good] = np.median(offset[good])
    rate[~timed] = np.median(rate[timed] if timed.any() else rate[good])
    print(f"carrier {f0:+.6f}: D0 {d0}, {len(found)} bursts, lengths {lengths.tolist()}; rate per item {rate.tolist()} (margin_db "
          f"{np.round(rates['margin_db'], 1).tolist()}), offset per item {offset.tolist()} (margin_db "
          f"{np.round(offsets['margin_db'], 1).tolist()})")
    return rows, lengths, rate, offset, d0


def receive_rows(pkg, rows, payloads):
    """test_blind_receive.packets_of_rows for rows of any width"""
    n = rows.shape[1]
    got = pkg.NativeMultiChannelReceiver(len(payloads), syncword_threshold=20.0, max_items=n).process_bulk(rows)
    tags = [int(got[r]["detector_tags"]["index"].size) for r in range(len(payloads))]
    good = []
    for r, payload in enumerate(payloads):
        rx = pkg.NativePacketReceiver(max_items=n, tags_cap=2048, packets_only=True, decode_headers=True, syncword_threshold=20.0)
        good.append(received_packets(rx.process_bulk(rows[r].contiguous())) == [payload])
    return tags, good


@pytest.mark.gpu
def test_one_carrier_blind_on_the_rows(pkg, scene_b):
    x, payloads = scene_b
    carriers = pkg.Spectrum().process_bulk(x).carriers()
    assert len(carriers) == 1
    rows, lengths, rate, offset, d0 = burst_rows(pkg, x, carriers[0])
    assert rows.shape[0] == B_BURSTS
    print(f"rate error per row {(rate / d0 / 0.04 - 1.0).tolist()}")
    y, out_lengths = pkg.RowResampler().to_samples_per_symbol(rows, lengths, rate, offset, n_cols=N_COLS)
    assert y.shape == (B_BURSTS, N_COLS) and int(out_lengths.max()) <= N_COLS
    tags, good = receive_rows(pkg, y, payloads)
    assert tags == [1] * B_BURSTS, f"detector tags per row {tags}"
    assert all(good), good


C2_CARRIER, C2_RATE, C2_FIRST_GAP = -0.21, 1.2345, 4200


@pytest.fixture(scope="module")
def scene_two(pkg, scene_b):
    """scene (b)'s stream plus a second carrier at 4 * 1.2345 * 5 = 24.69 wideband samples per symbol, under one noise"""
    import torch
    x1, payloads1 = scene_b
    rng = np.random.default_rng(2030)
    payloads2 = [rng.integers(0, 256, PAYLOAD, dtype=np.uint8).tobytes() for _ in range(B_BURSTS)]
    b, _, _ = pkg.PacketTransmitter().process_bulk(payloads2, gaps=[C2_FIRST_GAP] + [B_GAP] * (B_BURSTS - 1))
    v = torch.cat([b, torch.zeros(B_TAIL, dtype=torch.complex64, device="cuda")]).contiguous()
    u, consumed = pkg.PfbArbResampler(C2_RATE).process_bulk(v)
    assert consumed == v.numel()
    x2 = pkg.Duc([C2_CARRIER], 5, max_items=u.numel()).process_bulk(u[None, :].contiguous()).reshape(-1)
    n = max(x1.numel(), x2.numel())
    x = torch.zeros(n, dtype=torch.complex64, device="cuda")
    x[:x1.numel()] += x1  # carries scene (b)'s noise
    x[:x2.numel()] += x2
    return x.contiguous(), payloads1, payloads2


@pytest.mark.gpu
def test_two_carriers_of_non_simple_rates_in_one_call(pkg, scene_two):
    x, payloads1, payloads2 = scene_two
    carriers = pkg.Spectrum().process_bulk(x).carriers()
    assert len(carriers) == 2
    # which payloads belong to which found carrier; the frequencies in use are the found ones
    order = [int(np.argmin(np.abs(carriers["frequency"] - f))) for f in (B_CARRIER, C2_CARRIER)]
    assert sorted(order) == [0, 1]
    parts = [burst_rows(pkg, x, carriers[k]) for k in order]
    assert [p[0].shape[0] for p in parts] == [B_BURSTS, B_BURSTS]
    import torch
    rows = torch.cat([p[0] for p in parts])
    lengths = np.concatenate([p[1] for p in parts])
    rates = np.concatenate([p[2] for p in parts])
    offsets = np.concatenate([p[3] for p in parts])
    true = [0.04, 1.0 / (4 * C2_RATE * 5)]
    for k, p in enumerate(parts):
        print(f"carrier {k}: rate error per row {(p[2] / p[4] / true[k] - 1.0).tolist()}")
    try:
        i, d = pkg.resample_ratio(float(np.median(parts[1][2])) / parts[1][4])
        print(f"resample_ratio for the second carrier: {i} / {d}, a rate error of {i / d / (4 * true[1]) - 1.0:+.2e}")
    except pkg.Gr4pmError as e:
        print(f"resample_ratio for the second carrier raises: {e}")
    y, out_lengths = pkg.RowResampler().to_samples_per_symbol(rows, lengths, rates, offsets, n_cols=N_COLS)  # ONE call
    assert y.shape == (2 * B_BURSTS, N_COLS) and int(out_lengths.max()) <= N_COLS
    tags, good = receive_rows(pkg, y, payloads1 + payloads2)
    assert tags == [1] * (2 * B_BURSTS), f"detector tags per row {tags}"
    assert all(good), good


@pytest.mark.gpu
def test_the_file_app_receives_the_burst_rows(pkg, scene_b, tmp_path, capsys):
    """scene (a) as an sc16 file -> packet_receiver_file.py --burst-rows --tune auto --refine --decimate auto"""
    x, payloads = scene_b
    path, out = str(tmp_path / "wideband.sc16"), str(tmp_path / "packets.bin")
    xr = np.ascontiguousarray(x.cpu().numpy()).view(np.float32).reshape(-1, 2)
    assert np.abs(xr).max() * 4096.0 < 32767
    np.round(xr * 4096.0).astype("<i2").tofile(path)
    app = load_app("packet_receiver_file")
    app.main([path, "4", "20.0", "--format", "sc16", "--scale", str(1.0 / 4096.0), "--burst-rows", "--tune", "auto", "--refine",
              "--decimate", "auto", "--chunk-items", "200000", "--out", out])
    text = capsys.readouterr().out
    print(text)
    assert "--burst-rows:" in text and "no streaming pass over the file" in text
    assert "Msps" not in text  # receive_file's line: the streaming path did not run
    got, data, pos = [], open(out, "rb").read(), 0
    while pos < len(data):
        n = int.from_bytes(data[pos:pos + 2], "big")
        got.append(data[pos + 2:pos + 2 + n])
        pos += 2 + n
    assert got == payloads
