"""The loop Ddc.extract closes: the bursts a Spectrogram finds in a wideband recording are down-converted on their own,
one short row per burst, and received.

The scene is tests/test_spectrogram_bursts.py's, built again with the same constants and with its payloads kept: 3
carriers, 6 bursts each of 64-byte packets, I = 5, noise 0.05.  Spectrogram(hop=512, average=4) -> band_power -> bursts()
per carrier say WHEN; Ddc(CARRIERS, 5).burst_spans(found, k, margin_frames=ceil(row_span / 5)) -> extract() gives 18 rows;
NativeMultiChannelReceiver finds exactly one packet in every row and NativePacketReceiver returns that burst's payload
byte for byte.  The streaming path -- Ddc.process_bulk(x), cut at the same spans, zero-padded to the same n_cols -- is
held to the same two assertions first, so that a failure of the scene is not taken for one of the kernel.

The spans' times come from the spectrogram; the frequencies are the scene's known carriers, not the Spectrum's estimate:
find_carriers is only good to 1 / 2048 cycle per wideband sample, that is 0.0153 rad per wideband sample or 0.077 rad per
channel item, and the detector's +-4 bins reach +-0.042 rad per item.  A finer frequency estimate is a later issue.

n_cols = 6144: a multiple of 2048 and the smallest that holds the longest span.  A span is a burst of 1936 items, the
margin of 717 frames on either side, up to one row_span (717 items) of the burst finder's slack on either side, and
the 12 frames the filter's 60 taps add: up to about 4820 frames, more than 4096."""
import numpy as np
import pytest

from _frontend import bits, host, load_package, received_packets

I = 5
CARRIERS = [-0.37, 0.13, 0.41]
GAINS = [1.0, 0.5, 1.0]
BURSTS, PAYLOAD, GAP = 6, 64, 5000
FIRST_GAPS = [3000, 5200, 1100]
BURST = 4 * (4 * PAYLOAD + 228)  # items of one shaped burst at 4 samples per symbol
N = 50000
SIGMA = 0.05
HOP, R, FFT = 512, 4, 2048
ROW_SPAN = (R - 1) * HOP + FFT
MARGIN = -(-ROW_SPAN // I)  # frames
TAPS = 12 * I               # of the Ddc's default prototype
N_COLS = 6144


def truth(k):
    """[(a, e)]: burst b of row k covers the wideband samples [a, e)"""
    return [(I * (FIRST_GAPS[k] + b * (BURST + GAP)), I * (FIRST_GAPS[k] + b * (BURST + GAP) + BURST)) for b in range(BURSTS)]


def test_every_allowed_window_holds_its_burst_and_no_other():
    """from the known offsets alone: a found burst may begin and end anywhere within one row_span of the truth
    (test_spectrogram_bursts.assert_the_bursts).  The narrowest and the widest such window, widened by the margin of 717
    frames, give spans that contain the burst's items whole, that see no sample of a neighbouring burst of the same
    carrier (the gaps are 5000 items), and that fit n_cols."""
    import __graft_entry__ as ge
    span = ge.load_package().ddc_burst_span
    assert (ROW_SPAN, MARGIN) == (3584, 717)
    longest = 0
    for k in range(len(CARRIERS)):
        t = truth(k)
        for b, (a, e) in enumerate(t):
            for slack in (-(ROW_SPAN - 1), 0, ROW_SPAN - 1):  # the window is wider, exact, narrower than the truth
                first, n = span(a + slack, e - slack, I, TAPS, 0, MARGIN)
                last = first + n - 1
                assert first <= a // I and last >= (e - 1) // I, (k, b, slack)
                seen = (first * I + I - TAPS, last * I + I - 1)  # the samples its frames are made of
                for j, (a2, e2) in enumerate(t):
                    assert j == b or e2 <= seen[0] or a2 > seen[1], (k, b, j, slack)
                longest = max(longest, n)
    assert 4096 < longest <= N_COLS and N_COLS % 2048 == 0 and N_COLS - 2048 < longest
    assert max(FIRST_GAPS) + BURSTS * BURST + (BURSTS - 1) * GAP <= N


# ---- GPU ----

@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def scene(pkg):
    """the wideband stream [N I] on the device, the payloads per carrier, and the carriers a Spectrum finds in it"""
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
    assert len(carriers) == len(CARRIERS) and all(abs(float(c["frequency"]) - f) <= 1.0 / FFT for c, f in zip(carriers, CARRIERS))
    return x, sent, carriers


def assert_one_packet_per_row(pkg, rows, payloads, what):
    """exactly one detector tag in every row, and every row's packet is its burst's payload, byte for byte"""
    got = pkg.NativeMultiChannelReceiver(len(payloads), syncword_threshold=20.0, max_items=N_COLS).process_bulk(rows)
    tags = [got[r]["detector_tags"]["index"].size for r in range(len(payloads))]
    assert tags == [1] * len(payloads), f"{what}: detector tags per row {tags}"
    for r, payload in enumerate(payloads):
        rx = pkg.NativePacketReceiver(max_items=N_COLS, tags_cap=2048, packets_only=True, decode_headers=True, syncword_threshold=20.0)
        assert received_packets(rx.process_bulk(rows[r].contiguous())) == [payload], f"{what}: row {r}"


@pytest.mark.gpu
def test_found_bursts_are_extracted_and_received(pkg, scene):
    import torch
    x, sent, carriers = scene
    sg = pkg.Spectrogram(hop=HOP, average=R)
    assert sg.row_span == ROW_SPAN
    power = sg.band_power(sg.process_bulk(x), carriers)
    d = pkg.Ddc(CARRIERS, I)
    assert d.taps.size == TAPS
    spans, payloads = [], []
    for k in range(len(CARRIERS)):
        found = sg.bursts(power[k])
        assert len(found) == BURSTS, (k, len(found))
        spans += d.burst_spans(found, k, margin_frames=MARGIN)
        payloads += sent[k]
    assert len(spans) == 18 and N_COLS - 2048 < max(n for _, _, n in spans) <= N_COLS
    print("spans:", spans)

    # the streaming path, cut at the same spans and zero-padded to the same n_cols
    full = pkg.Ddc(CARRIERS, I).process_bulk(x)
    cut = torch.zeros((len(spans), N_COLS), dtype=torch.complex64, device="cuda")
    for r, (k, a, n) in enumerate(spans):
        piece = full[k, a:a + n]  # a span may run past the recording's end: there the stream is zero
        cut[r, :piece.numel()] = piece
    assert_one_packet_per_row(pkg, cut, payloads, "streaming path")

    rows, lengths = d.extract(x, spans, n_cols=N_COLS)
    assert tuple(rows.shape) == (18, N_COLS) and list(lengths) == [n for _, _, n in spans]
    assert_one_packet_per_row(pkg, rows, payloads, "extract")
    # and the rows are the stream's, bit for bit, wherever the stream has them
    rows_h, cut_h, F = host(rows), host(cut), full.shape[1]
    for r, (k, a, n) in enumerate(spans):
        m = min(n, F - a)
        assert np.array_equal(bits(rows_h[r, :m]), bits(cut_h[r, :m])) and not bits(rows_h[r, n:]).any(), r
