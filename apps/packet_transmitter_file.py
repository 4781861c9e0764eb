#!/usr/bin/env python3
"""MI355X counterpart of the reference's apps/packet_transmitter_pdu.cpp:

    packet_transmitter_file.py output_file (--in packets.bin | --random COUNT SIZE) [--stream-mode] [--gap N]
                               [--format {cf32,sc16,sc8,cu8}] [--gain G] [--tune CYCLES_PER_SAMPLE --interpolate N[/M]]
                               [--fft-duc]

makes the IQ of PacketTransmitterPdu (packet_transmitter_pdu.hpp:40-355) on the GPU (gr4pm_packet_transmitter) at
4 samples/symbol and writes it to `output_file` as raw little-endian complex64 (what packet_receiver_file.py reads).
The reference takes its packets from a TUN device; here they come from `--in`, a file of records of a big-endian uint16
length followed by the bytes (the format packet_receiver_file.py --out writes), or from `--random COUNT SIZE`: COUNT
packets of SIZE random bytes (`--seed`).

Burst mode (the default) writes `--gap` samples of silence in front of every burst; `--stream-mode` sends the packets
back to back through one continuous filter, without ramp-down, flush or burst shaping.

`--format sc16 | sc8 | cu8` writes interleaved little-endian int16, int8 or uint8 (I, Q) instead, what a DAC or
packet_receiver_file.py --format takes: packed on the device (gr4pm_iq_pack: rint(x * gain), cu8 around 127.5,
clamped; `--gain`: default 2^15 or 2^7).  The number of clipped components is printed at the end.  With `--tune` the
Duc or the FftDuc writes the integers itself (gr4pm_duc_process_iq / gr4pm_fft_duc_process_iq: the same bytes and count
without the complex64 band in between).

`--tune F --interpolate I`: the file is a wideband stream at I times the modem's rate with the carrier F cycles per file
sample off centre: a one-channel `Duc` (gr4pm_duc: interpolate by I, mix by +F) sits behind the
transmitter, and packet_receiver_file.py --tune F --decimate I receives the file.  Combines with `--format`; the
prototype's P - 1 items of tail are flushed, so the last burst's ramp-down is whole.  `--interpolate N/M` (N >= M, for
instance 25/4 for a 25 Msps file of a 1 Msym/s carrier): N / M file samples per transmitter sample, the same Duc
resampling by N / M in the same pass, so a file can be written at any rate above the modem's;
packet_receiver_file.py --tune F --decimate N/M receives it.

`--fft-duc` (with `--tune F --interpolate I`, I a power of two in 4 .. 64): the `FftDuc` (gr4pm_fft_duc: the same filter as
fast convolution) in the Duc's place, its flush() for the tail.  packet_receiver_file.py --tune F
--decimate I receives the file, and so does its --fft-ddc."""
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


def interpolation(v):
    """--interpolate: `N` or `N/M`, file samples per transmitter sample, as (N, M); an integer passes as (N, 1)"""
    n, _, m = str(v).partition("/")
    try:
        n, m = int(n), int(m) if m else 1
    except ValueError:
        raise ValueError(f"--interpolate: {v!r} is neither N nor N/M") from None
    if m < 1 or (m > 1 and n < m):
        raise ValueError(f"--interpolate: {v!r}: need N >= M >= 1 (file samples per transmitter sample)")
    return n, m  # a plain integer goes to the Duc as it is, which refuses what it cannot take


def transmit(packets, out_path, stream_mode=False, gap=0, batch=4096, pkg=None, fmt="cf32", gain=None, stats=None,
             tune=None, interpolate=None, fft_duc=False):
    """writes the IQ of `packets` to out_path; returns the number of samples written.  stats: an optional dict that
    receives "clipped", the number of components an integer format clipped.  tune / interpolate: a Duc behind the
    transmitter; interpolate: an integer, "N/M" or (N, M).  fft_duc: the FftDuc in its place (tune and an integer
    interpolate that the block takes)"""
    pkg = pkg or ge.load_package()
    clipped = None if fmt == "cf32" else torch.zeros(1, dtype=torch.int64, device="cuda")
    empty = [k for k, p in enumerate(packets) if len(p) == 0]
    if empty:  # PacketIngress refuses them (packet_ingress.hpp:171-172)
        raise ValueError(f"packets of length 0 at {empty[:5]}")
    batch_bytes = max([sum(len(p) for p in packets[i:i + batch]) for i in range(0, len(packets), batch)] + [1])
    tx = pkg.PacketTransmitter(stream_mode=stream_mode, samples_per_symbol=4, max_packets=batch,
                               max_payload_bytes=batch_bytes)
    duc = fast = None
    if tune is not None or interpolate is not None or fft_duc:
        up, down = (1, 1) if interpolate is None else (interpolate if isinstance(interpolate, tuple) else interpolation(interpolate))
        if fft_duc:
            if tune is None or interpolate is None or down != 1:
                raise ValueError("the FftDuc needs a carrier offset and an integer interpolation (--tune F --interpolate I)")
            fast = pkg.FftDuc([tune], up)
        else:
            duc = pkg.Duc([0.0 if tune is None else tune], up, decimation=down)
    written = 0

    # a bank behind the transmitter writes an integer format itself: no complex64 band, no second pass
    bank = {} if fmt == "cf32" else dict(format=fmt, gain=gain, clipped=clipped)

    def emit(f, x):
        if fast is not None:
            write(f, fast.process_bulk(x, **bank))
        elif duc is not None:
            for lo in range(0, x.numel(), duc.max_items):
                write(f, duc.process_bulk(x[lo:lo + duc.max_items], **bank))
        else:
            write(f, x if fmt == "cf32" else pkg.iq_pack(x, fmt, gain, clipped=clipped))

    def write(f, x):
        """x: complex64 [n], or the file's integer items [n, 2]"""
        nonlocal written
        written += x.shape[0]
        f.write(x.cpu().numpy().tobytes())

    with open(out_path, "wb") as f:
        for i in range(0, len(packets), batch):
            chunk = packets[i:i + batch]
            gaps = None if stream_mode else [gap] * len(chunk)
            x, _, _ = tx.process_bulk(chunk, gaps=gaps)
            emit(f, x)
        if fast is not None:  # whole segments: what the items so far still owe, the filter's tail included
            write(f, fast.flush(**bank))
        if duc is not None:  # the filter's tail
            emit(f, torch.zeros(len(duc.taps) // duc.interpolation + 1, dtype=torch.complex64, device="cuda"))
    if stats is not None and clipped is not None:
        stats["clipped"] = int(clipped.item())
    return written


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("output_file", help="raw complex64 IQ at 4 samples/symbol (times --interpolate)")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--in", dest="input_file", help="packets: uint16 big-endian length + bytes each")
    src.add_argument("--random", nargs=2, type=int, metavar=("COUNT", "SIZE"), help="COUNT random packets of SIZE bytes")
    ap.add_argument("--seed", type=int, default=1, help="of --random")
    ap.add_argument("--stream-mode", action="store_true", help="packets back to back, no bursts")
    ap.add_argument("--gap", type=int, default=0, help="samples of silence before each burst (burst mode)")
    ap.add_argument("--format", choices=["cf32", "sc16", "sc8", "cu8"], default="cf32", help="the file's items (default: complex64)")
    ap.add_argument("--gain", type=float, help="of an integer format's components (default: 2^15 for sc16, else 2^7)")
    ap.add_argument("--tune", type=float, metavar="CYCLES_PER_SAMPLE", help="the carrier's offset in the file (a Duc behind)")
    ap.add_argument("--interpolate", metavar="N[/M]", help="file samples per transmitter sample, an integer or a ratio N/M "
                    "such as 25/4 (a Duc behind)")
    ap.add_argument("--fft-duc", action="store_true", help="the FftDuc in the Duc's place: with --tune F --interpolate I, I a "
                    "power of two in 4 .. 64")
    a = ap.parse_args()
    if a.stream_mode and a.gap:
        ap.error("--gap is a burst mode option")
    if a.interpolate is not None:
        try:
            a.interpolate = interpolation(a.interpolate)
        except ValueError as e:
            ap.error(str(e))
    if a.fft_duc:
        if a.tune is None or a.interpolate is None:
            ap.error("--fft-duc needs --tune F --interpolate I")
        n, m = a.interpolate
        if m != 1 or n not in (4, 8, 16, 32, 64):
            ap.error(f"--fft-duc: --interpolate {n}{'/%d' % m if m != 1 else ''}: the FftDuc takes a power of two in 4 .. 64 "
                     "(and no ratio N/M); the Duc without --fft-duc takes the rest")
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
    stats = {}
    n = transmit(packets, a.output_file, a.stream_mode, a.gap, fmt=a.format, gain=a.gain, stats=stats,
                 tune=a.tune, interpolate=a.interpolate, fft_duc=a.fft_duc)
    print(f"{len(packets)} packets, {n} samples -> {a.output_file}" +
          (f" ({a.format}, {stats['clipped']} clipped components)" if "clipped" in stats else ""))


if __name__ == "__main__":
    main()
