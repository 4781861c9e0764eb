#!/usr/bin/env python3
"""Packet error rate over an Es/N0 sweep: PacketTransmitter -> Channel (PfbArbResampler for the SFO, Rotator for the
CFO, Gaussian NoiseSource added, apps/packet_transceiver.cpp:48-78) -> NativePacketReceiver(packets_only).

    packet_error_rate.py [--esn0 4:18:2] [--packets 2000] [--size 1500] [--stream] [--cfo 0] [--sfo-ppm 0]
                         [--seed 0] [--json out.json]

--esn0 lo:hi:step (hi included) or a comma list.  Each point sends --packets random packets of --size bytes, in calls
of --batch packets through one channel and one receiver, and counts a packet as received when its bytes come back
exact.  PER = 1 - received / sent.  Header loss = 1 - (valid headers whose length is the one sent) / sent; the count of
all valid headers is printed beside it, so false detections that decode as valid stay visible.  By default each point is one
call: a packet cut by a call boundary is not delivered by this driver (it hands the receiver no history), so --batch
below --packets counts a few such cuts as lost at every Es/N0."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def parse_points(s):
    if ":" in s:
        lo, hi, step = (float(v) for v in s.split(":"))
        return [float(v) for v in np.arange(lo, hi + step / 2, step)]
    return [float(v) for v in s.split(",")]


def run_point(pkg, esn0, a):
    rng = np.random.default_rng(a.seed)
    tx = pkg.PacketTransmitter(stream_mode=a.stream, max_packets=a.batch, max_payload_bytes=a.batch * a.size)
    ch = pkg.Channel(samples_per_symbol=4, esn0_db=esn0, cfo=a.cfo, sfo_ppm=a.sfo_ppm, seed=a.seed,
                     max_items=tx.output_items([a.size] * a.batch) + (1 << 16))
    rx = pkg.NativePacketReceiver(max_items=tx.output_items([a.size] * a.batch) + (1 << 16), tags_cap=4 * a.batch + 64,
                                  decode_headers=True, packets_only=True)
    sent, got, headers, matching = 0, 0, 0, 0
    pending = set()
    left = a.packets
    while left > 0:
        k = min(a.batch, left)
        payloads = [rng.integers(0, 256, a.size, dtype=np.uint8).tobytes() for _ in range(k)]
        x, _, _ = tx.process_bulk(payloads)
        if left == k:  # the last call: flush the receiver with silence
            x = torch.cat([x, torch.zeros(1 << 14, dtype=torch.complex64, device=x.device)])
        y = ch.process_bulk(x)
        r = rx.process_bulk(y)
        pending |= set(payloads)
        sent += k
        left -= k
        hm = r["header_messages"]
        valid = hm["invalid_header"] == 0
        headers += int(np.count_nonzero(valid))
        matching += int(np.count_nonzero(valid & (hm["packet_length"] == a.size)))
        data, lens = r["packets"].cpu().numpy(), r["packet_lengths"]
        pos = 0
        for n in lens[lens > 0]:
            p = data[pos:pos + int(n)].tobytes()
            pos += int(n)
            if p in pending:
                pending.discard(p)
                got += 1
    # header loss counts only valid headers that carry the length sent; more of them than packets (false detections
    # that decode as valid) shows as a negative loss, not as zero
    return {"esn0_db": esn0, "sent": sent, "received": got, "per": 1.0 - got / sent, "valid_headers": headers,
            "matching_headers": matching, "header_loss": 1.0 - matching / sent, "noise_amplitude": ch.noise_amplitude,
            "n0": ch.n0}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--esn0", default="4:18:2")
    ap.add_argument("--packets", type=int, default=2000)
    ap.add_argument("--size", type=int, default=1500)
    ap.add_argument("--batch", type=int, default=0, help="packets per call (default: all in one call)")
    ap.add_argument("--stream", action="store_true", help="stream mode (default: burst mode)")
    ap.add_argument("--cfo", type=float, default=0.0, help="rad/sample")
    ap.add_argument("--sfo-ppm", type=float, default=0.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json")
    a = ap.parse_args()
    a.batch = a.batch or a.packets
    if not torch.cuda.is_available():
        sys.exit("packet_error_rate.py needs a GPU")
    pkg = ge.load_package()
    rows = []
    print(f"{'stream' if a.stream else 'burst'} mode, {a.size}-byte packets, cfo {a.cfo} rad/sample, sfo {a.sfo_ppm} ppm")
    print(f"{'Es/N0 dB':>8} {'sent':>6} {'received':>8} {'PER':>10} {'valid hdrs':>10} {'header loss':>12}")
    for esn0 in parse_points(a.esn0):
        r = run_point(pkg, esn0, a)
        rows.append(r)
        print(f"{esn0:8.1f} {r['sent']:6d} {r['received']:8d} {r['per']:10.3e} {r['valid_headers']:10d} "
              f"{r['header_loss']:12.3e}", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
