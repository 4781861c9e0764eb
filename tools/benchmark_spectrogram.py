#!/usr/bin/env python3
"""Rate of the Spectrogram block (csrc/spectrogram.hip) beside the Spectrum at the same hop and a copy of the same bytes,
and of band_power beside a read of the same bytes, all in the same process.

  tools/benchmark_spectrogram.py [--log2-items 28] [--iters 20]

One process_bulk() call of 2^log2-items wideband samples per iteration, timed with device events; the median over the
iterations, in Gsamples/s of input, for hop 2048 and 1024, average R = 1 and 16, and complex64 and sc16 input.  Beside
each: Spectrum.process_bulk() of the same input at the same hop, and torch's device-to-device copy of the input's bytes
(8 or 4 read and as many written per sample; the Spectrogram reads them and writes 4 hop^-1 R^-1 2048 bytes of rows per
sample).  Prints one JSON line per (hop, R, format).  Then band_power() for 3 bands on the R = 1 rows of each hop beside
a torch sum over the same rows (a read of the same bytes), one JSON line per hop.  Expected from the code, not asserted:
at R = 16 the kernel does the Spectrum's work per segment with a sixteenth of a row store per segment, so its time is
close to the Spectrum's; at R = 1 and hop 2048 it also stores 4 bytes per sample."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchmark_channelizer import median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2-items", type=int, default=28)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    assert torch.cuda.is_available(), "needs a GPU"
    n = 1 << args.log2_items
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.randn((n, 2), dtype=torch.float32, device="cuda", generator=g))
    xi = pkg.iq_pack(x, "sc16", 0.125 * 32768.0)
    device = torch.cuda.get_device_name(0)
    copies = {}
    for name, src in (("cf32", x), ("sc16", xi)):
        dst = torch.empty_like(src)
        copies[name] = median_ms(lambda: dst.copy_(src), args.iters, torch)
        del dst
    bands = [(100, 138), (2000, 138), (900, 70)]
    for hop in (2048, 1024):
        sp = pkg.Spectrum(hop=hop)
        spectrum_ms = {name: median_ms(lambda: sp.process_bulk(src), args.iters, torch) for name, src in (("cf32", x), ("sc16", xi))}
        for R in (1, 16):
            sg = pkg.Spectrogram(hop=hop, average=R)

            def call(src):
                sg.reset()  # every iteration is the same call: the same rows
                return sg.process_bulk(src)

            for name, src, item_bytes in (("cf32", x, 8), ("sc16", xi, 4)):
                ms = median_ms(lambda: call(src), args.iters, torch)
                rows = sg.rows_done
                gsps = n / ms / 1e6
                print(json.dumps({"tool": "benchmark_spectrogram", "hop": hop, "average": R, "format": name, "items": n,
                                  "rows": rows, "ms": round(ms, 4), "gsamples_per_s": round(gsps, 2),
                                  "read_tb_per_s": round(item_bytes * gsps / 1e3, 3),
                                  "write_tb_per_s": round(rows * 2048 * 4 / ms / 1e9, 3),
                                  "spectrum_ms": round(spectrum_ms[name], 4), "over_spectrum": round(ms / spectrum_ms[name], 3),
                                  "copy_ms": round(copies[name], 4), "over_copy": round(ms / copies[name], 3), "device": device}))
            if R == 1:
                rows = call(x)
                ms = median_ms(lambda: sg.band_power(rows, bands), args.iters, torch)
                read_ms = median_ms(lambda: rows.sum(dim=1), args.iters, torch)
                print(json.dumps({"tool": "benchmark_spectrogram", "what": "band_power", "hop": hop, "rows": rows.shape[0],
                                  "bands": len(bands), "ms": round(ms, 4), "read_tb_per_s": round(rows.numel() * 4 / ms / 1e9, 3),
                                  "torch_row_sum_ms": round(read_ms, 4), "over_torch_row_sum": round(ms / read_ms, 3),
                                  "device": device}))
                del rows


if __name__ == "__main__":
    main()
