#!/usr/bin/env python3
"""Receives several carriers of different symbol rates from one wideband recording of any length, in one pass.

  band_receiver_file.py wide.sc16 --format sc16 --carrier FREQ:DECIMATION:SYMBOLS_PER_SAMPLE [--carrier ...]
  band_receiver_file.py wide.sc16 --format sc16 --scan
      [--chunk-items N] [--out-prefix P] [--scale S] [syncword_freq_bins] [syncword_threshold]

Every chunk of the file goes through one chain:
  MixedFftDdc.process_bulk      one forward transform per segment, a power-of-two decimation per carrier
  StreamRowResampler            every row to exactly 4 samples per symbol at any real ratio, its residual offset removed,
                                position, history and phase carried from chunk to chunk
  RowPacketReceivers            one receiver per row, which keeps what its receiver has not consumed yet
and the flushes follow at the end, so the chunk size changes no packet.

--carrier FREQ:DECIMATION:SYMBOLS_PER_SAMPLE (repeatable): the carrier's centre in cycles per file sample, the MixedFftDdc's
decimation for it (4, 8, 16, 32 or 64) and its symbol rate in symbols per file sample.  A frequency below zero is written
with an equals sign: --carrier=-0.31:4:0.05.
--scan: the first chunk is scanned as packet_receiver_file.py --scan does (Spectrum().carriers()); every carrier gets the
decimation fft_ddc_decimation() makes of its bandwidth (a carrier it refuses is printed and skipped) and is looked at through
a LineSpectrum on its bursts (packet_receiver_file.refine_file): the residual offset is added to the scan's frequency, the
symbol rate is the carrier's (a carrier without a reading is printed and skipped).

--out-prefix P writes P.<k>.bin per carrier, uint16 big-endian length + bytes per packet, packet_receiver_file.py's --out
format.  One line per carrier is printed."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import packet_receiver_file as prf  # noqa: E402  (sets the process up as that app does, before torch is imported)

import torch  # noqa: E402

ge = prf.ge


def carrier_value(v):
    """--carrier: FREQ:DECIMATION:SYMBOLS_PER_SAMPLE as (float, int, float)"""
    try:
        f, d, r = str(v).split(":")
        f, d, r = float(f), int(d), float(r)
    except ValueError:
        raise ValueError(f"--carrier: {v!r} is not FREQ:DECIMATION:SYMBOLS_PER_SAMPLE") from None
    if d not in (4, 8, 16, 32, 64) or not 0.0 < r * d <= 0.25:
        raise ValueError(f"--carrier: {v!r}: the decimation is 4, 8, 16, 32 or 64 and leaves the row 4 samples per symbol or more")
    return f, d, r


def scan_carriers(path, fmt, scale, chunk_items, pkg):
    """the carriers of the file's first chunk as (frequency, decimation, symbols per file sample)"""
    found, spectrum, items = prf.scan_file(path, fmt, scale, chunk_items, chunk_items, pkg)
    prf.print_carriers(found, spectrum, items)
    out = []
    for c in found:
        f, bw = float(c["frequency"]), float(c["bandwidth"])
        try:
            d = pkg.fft_ddc_decimation(bw)
        except pkg.Gr4pmError as e:
            print(f"carrier {f:+.6f}: skipped: {e}")
            continue
        r = prf.refine_file(path, f, bw, fmt, scale, chunk_items, chunk_items, pkg)
        if r["rate"] is None:
            print(f"carrier {f:+.6f}: skipped: none of the {r['rows']} rows at decimation {r['decimation']} shows a carrier line "
                  "to read the symbol rate beside")
            continue
        print(f"carrier {f:+.6f}: offset {r['offset']:+.3e}, {r['rate']:.7f} symbols per file sample, decimation {d}")
        out.append((f + r["offset"], d, r["rate"]))
    return out


def receive_band(path, carriers, fmt="cf32", scale=None, chunk_items=1 << 22, out_prefix=None, syncword_freq_bins=4,
                 syncword_threshold=9.5, pkg=None):
    """carriers: (frequency, decimation, symbols per file sample) each.  Returns dict(packets: a list of bytes per carrier,
    stats: RowPacketReceivers' per carrier, items, seconds)"""
    pkg = pkg or ge.load_package()
    K = len(carriers)
    rates = [r * d for _, d, r in carriers]  # symbols per row item
    ddc = pkg.MixedFftDdc([f for f, _, _ in carriers], [d for _, d, _ in carriers])
    rs = pkg.StreamRowResampler.for_rates(rates, max_step=max(1.0, max(1.0 / (4.0 * r) for r in rates)))
    rx = pkg.RowPacketReceivers(K, max_items=max(1 << 16, chunk_items), syncword_freq_bins=syncword_freq_bins,
                                syncword_threshold=syncword_threshold)
    packets = [[] for _ in range(K)]

    def behind(rows, lengths):
        for k, got in enumerate(rx.process_rows(rows, lengths)):
            packets[k] += got

    t0, items = time.perf_counter(), 0
    kw = {} if fmt == "cf32" else dict(scale=scale)
    for x in prf.file_chunks(path, fmt, None, chunk_items):
        items += x.shape[0]
        behind(*rs.process_rows(*ddc.process_bulk(x, **kw)))
    behind(*rs.flush())
    for k, got in enumerate(rx.flush()):
        packets[k] += got
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if out_prefix:
        for k in range(K):
            with open(f"{out_prefix}.{k}.bin", "wb") as f:
                for p in packets[k]:
                    f.write(len(p).to_bytes(2, "big"))
                    f.write(p)
    return {"packets": packets, "stats": rx.stats, "items": items, "seconds": dt}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("input_file")
    ap.add_argument("syncword_freq_bins", nargs="?", type=int, default=4)
    ap.add_argument("syncword_threshold", nargs="?", type=float, default=9.5)
    ap.add_argument("--format", choices=list(prf.FILE_DTYPES), default="cf32", help="the file's items (default: complex64)")
    ap.add_argument("--scale", type=float, help="of an integer format's components (default: 2^-15 for sc16, else 2^-7)")
    ap.add_argument("--carrier", type=carrier_value, action="append", metavar="FREQ:DECIMATION:SYMBOLS_PER_SAMPLE",
                    help="a carrier: centre in cycles per file sample, the decimation of its row (4 .. 64, a power of two), "
                         "symbols per file sample; repeatable")
    ap.add_argument("--scan", action="store_true", help="find the carriers, their offsets and symbol rates in the first chunk")
    ap.add_argument("--chunk-items", type=int, default=1 << 22)
    ap.add_argument("--out-prefix", metavar="P", help="write carrier k's packets to P.<k>.bin (uint16 big-endian length + bytes each)")
    a = ap.parse_args(argv)
    if bool(a.carrier) == bool(a.scan):
        ap.error("give --carrier (one or more) or --scan")
    pkg = ge.load_package()
    carriers = a.carrier or scan_carriers(a.input_file, a.format, a.scale, a.chunk_items, pkg)
    if not carriers:
        sys.exit("--scan: no carrier to receive")
    if len(carriers) > 64:
        sys.exit(f"{len(carriers)} carriers: one pass takes 64")
    r = receive_band(a.input_file, carriers, a.format, a.scale, a.chunk_items, a.out_prefix, a.syncword_freq_bins,
                     a.syncword_threshold, pkg)
    for k, ((f, d, rate), s) in enumerate(zip(carriers, r["stats"])):
        print(f"carrier {k} frequency {f:+.7f} decimation {d} symbols_per_sample {rate:.7f}: headers {s['headers']} "
              f"({s['invalid_headers']} invalid), packets {len(r['packets'][k])} ({s['crc_failures']} CRC failures), "
              f"{sum(len(p) for p in r['packets'][k])} bytes")
    print(f"{r['items']} samples in {r['seconds']:.3f} s = {r['items'] / r['seconds'] / 1e6:.1f} Msps (file and PCIe included)")


if __name__ == "__main__":
    main()
