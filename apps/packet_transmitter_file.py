#!/usr/bin/env python3
"""MI355X counterpart of the reference's apps/packet_transmitter_pdu.cpp:

    packet_transmitter_file.py output_file (--in packets.bin | --random COUNT SIZE) [--stream-mode] [--gap N]

makes the IQ of PacketTransmitterPdu (packet_transmitter_pdu.hpp:40-355) on the GPU (gr4pm_packet_transmitter) at
4 samples/symbol and writes it to `output_file` as raw little-endian complex64 (what packet_receiver_file.py reads).
The reference takes its packets from a TUN device; here they come from `--in`, a file of records of a big-endian uint16
length followed by the bytes (the format packet_receiver_file.py --out writes), or from `--random COUNT SIZE`: COUNT
packets of SIZE random bytes (`--seed`).

Burst mode (the default) writes `--gap` samples of silence in front of every burst; `--stream-mode` sends the packets
back to back through one continuous filter, without ramp-down, flush or burst shaping."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def read_packets(path):
    """records of a big-endian uint16 length followed by the bytes"""
    data, packets, pos = open(path, "rb").read(), [], 0
    while pos + 2 <= len(data):
        n = int.from_bytes(data[pos:pos + 2], "big")
        if pos + 2 + n > len(data):
            raise ValueError(f"{path}: truncated record at byte {pos}")
        packets.append(data[pos + 2:pos + 2 + n])
        pos += 2 + n
    return packets


def transmit(packets, out_path, stream_mode=False, gap=0, batch=4096, pkg=None):
    """writes the IQ of `packets` to out_path; returns the number of samples written"""
    pkg = pkg or ge.load_package()
    empty = [k for k, p in enumerate(packets) if len(p) == 0]
    if empty:  # PacketIngress refuses them (packet_ingress.hpp:171-172)
        raise ValueError(f"packets of length 0 at {empty[:5]}")
    batch_bytes = max([sum(len(p) for p in packets[i:i + batch]) for i in range(0, len(packets), batch)] + [1])
    tx = pkg.PacketTransmitter(stream_mode=stream_mode, samples_per_symbol=4, max_packets=batch,
                               max_payload_bytes=batch_bytes)
    written = 0
    with open(out_path, "wb") as f:
        for i in range(0, len(packets), batch):
            chunk = packets[i:i + batch]
            gaps = None if stream_mode else [gap] * len(chunk)
            x, _, _ = tx.process_bulk(chunk, gaps=gaps)
            f.write(x.cpu().numpy().tobytes())
            written += x.numel()
    return written


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("output_file", help="raw complex64 IQ at 4 samples/symbol")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--in", dest="input_file", help="packets: uint16 big-endian length + bytes each")
    src.add_argument("--random", nargs=2, type=int, metavar=("COUNT", "SIZE"), help="COUNT random packets of SIZE bytes")
    ap.add_argument("--seed", type=int, default=1, help="of --random")
    ap.add_argument("--stream-mode", action="store_true", help="packets back to back, no bursts")
    ap.add_argument("--gap", type=int, default=0, help="samples of silence before each burst (burst mode)")
    a = ap.parse_args()
    if a.stream_mode and a.gap:
        ap.error("--gap is a burst mode option")
    if a.random:
        count, size = a.random
        if not 1 <= size <= 65535:
            ap.error("SIZE must be in [1, 65535]")
        rng = np.random.default_rng(a.seed)
        packets = [rng.integers(0, 256, size, dtype=np.uint8).tobytes() for _ in range(count)]
    else:
        packets = read_packets(a.input_file)
    if not torch.cuda.is_available():
        sys.exit("packet_transmitter_file.py needs a GPU")
    n = transmit(packets, a.output_file, a.stream_mode, a.gap)
    print(f"{len(packets)} packets, {n} samples -> {a.output_file}")


if __name__ == "__main__":
    main()
