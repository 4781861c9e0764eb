"""The scene of tests/test_fft_filter_notch.py and tests/test_fft_filter_app.py: six bursts of the packet transmitter, noise,
and a CW interferer inside the channel, with the notch that removes it."""
import numpy as np

from _frontend import dev, host, received_packets

CW_FREQUENCY, NOTCH_WIDTH, NOTCH_TAPS, NOTCH_DB = 0.05, 0.012, 1025, 60.0
# the smallest of 2, 5, 10, 30 at which the receiver without the filter delivers fewer than six packets on the MI355X: it
# delivers 0 of 6 at every one of the four, and all 6 with the filter; the notch band's power falls by 64.5 dB at each
CW_AMPLITUDE = 2.0
ZERO_TAIL = 8192


def scene(pkg, amplitude=CW_AMPLITUDE, seed=2032):
    """(payloads, complex64 samples): 6 packets of 64 seeded bytes with gaps of 4000 at 4 samples per symbol and one more
    gap behind the last burst (the notch delays by (NOTCH_TAPS - 1) / 2 samples and delivers as many samples as it takes:
    without it the filtered stream would end inside the last burst), noise of sigma 0.05, and amplitude * exp(2 pi j 0.05 n)"""
    rng = np.random.default_rng(seed)
    payloads = [rng.integers(0, 256, 64, dtype=np.uint8).tobytes() for _ in range(6)]
    x, _, _ = pkg.PacketTransmitter(samples_per_symbol=4, max_packets=16).process_bulk(payloads, gaps=[4000] * 6)
    x = np.concatenate([host(x).astype(np.complex128), np.zeros(4000, np.complex128)])
    n = np.arange(x.size)
    x += 0.05 * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size)) / np.sqrt(2.0)
    x += amplitude * np.exp(2j * np.pi * CW_FREQUENCY * n)
    return payloads, x.astype(np.complex64)


def notch(pkg):
    """notch_taps of one band (0.05, width 0.012): a carrier record 0.008 wide, widened by 1.5"""
    carrier = np.array([(CW_FREQUENCY, NOTCH_WIDTH / 1.5)], dtype=[("frequency", "f8"), ("bandwidth", "f8")])
    return pkg.notch_taps(carrier, widen=1.5, n_taps=NOTCH_TAPS, attenuation_db=NOTCH_DB)


def filtered(pkg, x, taps, call=4097):
    """x through an FftFilter in calls of `call` samples, flushed; on the device"""
    import torch
    f = pkg.FftFilter(taps)
    xd = dev(x)
    parts = [f.process_bulk(xd[lo:lo + call]) for lo in range(0, x.size, call)]
    parts.append(f.flush())
    return torch.cat(parts)


def receive(pkg, y):
    """the packets the receiver delivers for the device stream y with a zero tail"""
    import torch
    z = torch.cat([y, torch.zeros(ZERO_TAIL, dtype=torch.complex64, device=y.device)])
    rx = pkg.NativePacketReceiver(max_items=z.numel(), tags_cap=2048, decode_headers=True, packets_only=True)
    return received_packets(rx.process_bulk(z))


def notch_band_power(pkg, y):
    """the power of the device stream y in the notch band, from a Spectrum's mean: the bins whose Hann main lobe (two bins
    either side) lies inside the band less half a transition width at each edge, where the design holds its attenuation"""
    mean = pkg.Spectrum().process_bulk(y).read()["mean"]
    half = 0.5 * NOTCH_WIDTH - 0.5 * (NOTCH_DB - 7.95) / (14.36 * (NOTCH_TAPS - 1))
    lo = int(np.ceil((CW_FREQUENCY - half) * 2048)) + 2
    hi = int(np.floor((CW_FREQUENCY + half) * 2048)) - 2
    assert hi - lo >= 8
    return float(mean[lo:hi + 1].sum())
