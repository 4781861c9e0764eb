#!/usr/bin/env python3
"""benchmarks/benchmark_packet_transmitter_pdu.cpp restated for gr4pm_packet_transmitter: 1500-byte zero packets at
4 samples/symbol, burst mode (stream_mode 0) or stream mode (1).

    benchmark_packet_transmitter.py [stream_mode ...] [--log2-packets 10 12 14] [--iters 10] [--json out.json]

Every call is timed whole (host checks, the packet table upload, the pre-pass and the sample kernel, the closing
stream synchronise) with device events, after two warm-up calls of the same shape.  The rate is output samples per
second; "of_store_ceiling" sets the 8 bytes written per sample against 6.0 TB/s, the MI355X's plain-store rate.  The
payload is read once by the pre-pass and once more by the sample kernel (1500 bytes per ~25 000 samples): not counted."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

STORE_CEILING = 6.0e12  # bytes/s


def run(pkg, stream_mode, n_packets, iters, packet_size=1500, sps=4):
    tx = pkg.PacketTransmitter(stream_mode=stream_mode, samples_per_symbol=sps, max_packets=n_packets,
                               max_payload_bytes=n_packets * packet_size)
    payload = torch.zeros(n_packets * packet_size, dtype=torch.uint8, device="cuda")
    lengths = np.full(n_packets, packet_size, dtype=np.uint64)
    n_out = tx.output_items(lengths)
    out = torch.empty(n_out, dtype=torch.complex64, device="cuda")
    for _ in range(2):
        tx.process_bulk(payload, lengths=lengths, out=out)
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        x, _, _ = tx.process_bulk(payload, lengths=lengths, out=out)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    assert x.numel() == n_out
    t = float(np.median(times))
    return {"stream_mode": int(stream_mode), "packets_per_call": n_packets, "samples_per_call": n_out,
            "seconds_median": t, "seconds_min": float(np.min(times)), "seconds_max": float(np.max(times)),
            "msamples_per_s": n_out / t / 1e6, "of_store_ceiling": 8 * n_out / t / STORE_CEILING}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("stream_mode", nargs="*", type=int, default=[0, 1])
    ap.add_argument("--log2-packets", nargs="+", type=int, default=[10, 12, 14])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", help="also write the results here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("benchmark_packet_transmitter.py needs a GPU")
    pkg = ge.load_package()
    results = []
    for mode in a.stream_mode:
        for lg in a.log2_packets:
            r = run(pkg, bool(mode), 1 << lg, a.iters)
            results.append(r)
            print(f"stream_mode {mode}  2^{lg} packets/call  {r['samples_per_call']:>11d} samples  "
                  f"{r['seconds_median'] * 1e3:8.3f} ms  {r['msamples_per_s']:10.1f} Msps  "
                  f"{100 * r['of_store_ceiling']:5.1f} % of the store ceiling", flush=True)
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
