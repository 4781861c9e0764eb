"""The blind burst path over a stream, on the GPU: the scene of tests/test_row_stream_carriers.py (two carriers of 20 and 25
wideband samples per symbol, 16 and 12 bursts, noise of 0.05) through MixedFftDdc -> RowBurstGate -> LineSpectrum ->
RowResampler -> one receiver per burst row, in calls of 4097, of 65 536 and of all samples, with the floors measured once
from the whole rows.  Exactly 16 and 12 bursts per carrier, none truncated, none dropped; the burst rows are the same bytes in
all three runs; every payload arrives byte for byte.  No symbol rate is given to the chain: each burst row's own line
spectra give its rate and offset.

The floor and the burst level per row item are the 0.1 and 0.9 quantiles of the block powers of 64 items, which the test
prints.  Measured on MI355X, both carriers at decimation 4: floor 5.03e-4 and 5.04e-4 per item, burst level 0.327 and 0.328,
28.1 dB above the floor.  So the defaults of set_floor (10 dB to open, 6 dB to stay open) separate them with 18 dB to
spare and are used as they are, and so are the margins of 4 blocks on either side: the burst rows are 2880 .. 2944 items
(carrier 0, bursts of 2420) and 3520 .. 3584 items (carrier 1, bursts of 3025), and every packet arrives."""
import numpy as np
import pytest

import test_row_stream_carriers as band
from _frontend import load_package

pytestmark = pytest.mark.gpu

CALLS = [4097, 65536, band.WIDE]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def receive_rows(pkg, rows, lengths, decimations, carrier_of, ls, rs):
    """burst rows -> (packets per burst row, the measured rates); a row without a trustworthy line takes the call's median"""
    D = np.array([decimations[k] for k in carrier_of], dtype=np.float64)
    offsets = ls.carrier_offset(rows, lengths, max_offset=float(min(0.1, 4.0 * D.min() / 2048)))
    rates = ls.symbol_rate(rows, lengths)
    good = (offsets["margin_db"] >= 6.0) & (rates["margin_db"] >= 6.0)
    rate, offset = rates["rate"].copy(), offsets["offset"].copy()
    for k in set(carrier_of):
        mine = np.array(carrier_of) == k
        if (mine & good).any():
            rate[mine & ~good] = np.median(rate[mine & good])
            offset[mine & ~good] = np.median(offset[mine & good])
    longest = int(rs.output_lengths(lengths, rs.steps_for(rate)).max())
    n_cols = (-(-longest // 2048) + 1) * 2048  # a block of zeros behind the longest row: the receiver delivers behind it
    y, _ = rs.to_samples_per_symbol(rows, lengths, rate, offset, n_cols=n_cols)
    packets = []
    for r in range(y.shape[0]):
        rx = pkg.NativePacketReceiver(4, 4, 20.0, max_items=n_cols, tags_cap=n_cols // 768 + 64, decode_headers=True, packets_only=True)
        res = rx.process_bulk(y[r].contiguous())
        data, pos, got = res["packets"].cpu().numpy(), 0, []
        for n in res["packet_lengths"][res["packet_lengths"] > 0]:
            got.append(data[pos:pos + int(n)].tobytes())
            pos += int(n)
        packets.append(got)
    return packets, rate


def receive(pkg, x, call, decimations, floors):
    """(packets per carrier, burst rows per carrier as bytes, records per carrier, the gate)"""
    import torch
    ddc = pkg.MixedFftDdc(band.CARRIERS, decimations)
    gate = pkg.RowBurstGate(2)
    gate.set_floor(floors)
    ls, rs = pkg.LineSpectrum(hop=256), pkg.RowResampler(max_step=2.0)
    packets, rows_of, records = [[], []], [[], []], [[], []]

    def behind(burst_rows, lengths, rec):
        if not len(rec):
            return
        got, _ = receive_rows(pkg, burst_rows, lengths, decimations, [int(r) for r in rec["row"]], ls, rs)
        host = burst_rows.cpu().numpy()
        for j, r in enumerate(rec["row"]):
            packets[r] += got[j]
            rows_of[r].append(host[j].tobytes())
            records[r].append(rec[j])

    for lo in range(0, band.WIDE, call):
        rows, lengths = ddc.process_bulk(x[lo:lo + call])
        if lengths.any():
            behind(*gate.process_rows(rows, lengths))
    behind(*gate.flush())
    torch.cuda.synchronize()
    return packets, rows_of, records, gate


def test_two_carriers_without_their_rates_in_any_cutting(pkg):
    x, sent = band.build_scene(pkg)
    decimations = [pkg.fft_ddc_decimation(1.35 / s) for s in band.PER_SYMBOL]
    rows, lengths = pkg.MixedFftDdc(band.CARRIERS, decimations).process_bulk(x)
    probe = pkg.RowBurstGate(2)
    floors = probe.measure_floor(rows, lengths)
    for k, sums in enumerate(probe.block_power(rows, lengths)):
        level = float(np.sort(sums)[int(0.9 * sums.size)]) / probe.block
        print(f"carrier {k}: decimation {decimations[k]}, floor {floors[k]:.3e} per item, burst level {level:.3e} "
              f"({10 * np.log10(level / floors[k]):.1f} dB above it), {sums.size} blocks")
        assert level > floors[k] * 10.0 ** 1.6, "10 dB and 6 dB above the floor leave no room below the bursts"
    first = None
    for call in CALLS:
        packets, rows_of, records, gate = receive(pkg, x, call, decimations, floors)
        for k in range(2):
            s = gate.state(k)
            assert (s["emitted"], s["dropped"], s["truncated"]) == (band.BURSTS[k], 0, 0), (call, k, s)
            assert len(records[k]) == band.BURSTS[k] and all(r["flags"] == 0 for r in records[k]), (call, k)
            assert packets[k] == sent[k], (call, k, len(packets[k]), len(sent[k]))
        if first is None:
            first, first_records = rows_of, records
            for k in range(2):
                n = [int(r["n_items"]) for r in records[k]]
                print(f"carrier {k}: burst rows of {min(n)} .. {max(n)} items")
        for k in range(2):
            assert rows_of[k] == first[k], (call, k)
            assert [r.tobytes() for r in records[k]] == [r.tobytes() for r in first_records[k]], (call, k)
