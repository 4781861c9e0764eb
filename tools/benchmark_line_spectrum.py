#!/usr/bin/env python3
"""Rate of the LineSpectrum block (csrc/line_spectrum.hip) against the Spectrum over the same bytes and a copy of them,
all in the same process.

  tools/benchmark_line_spectrum.py [--rows 64] [--log2-cols 22] [--iters 20]

One process_rows() call (normalize=False: the kernels alone) over [rows, 2^log2-cols] complex64 per iteration, timed with
device events; the median over the iterations, for the three statistics at hop 2048 and 1024.  Beside each: one
Spectrum.process_bulk() over the same bytes as one stream at the same hop, and torch's device-to-device copy of them (8
bytes read and 8 written per item; the spectra only read).  Then the shape Ddc.extract makes: 64 rows of 6144 items, where
a call is two launches of a few hundred waves.  Prints one JSON line per (shape, hop, statistic).  Expected from the
code, not asserted: the envelope at hop 2048 runs half of the Spectrum's transforms over the same bytes and should not take
longer than it; the fourth power runs the same transforms plus a few products per item and should be within a small
margin of it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchmark_channelizer import median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--log2-cols", type=int, default=22)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    assert torch.cuda.is_available(), "needs a GPU"
    g = torch.Generator(device="cuda").manual_seed(1)
    for rows, cols in ((args.rows, 1 << args.log2_cols), (64, 6144)):
        x = torch.view_as_complex(torch.randn((rows, cols, 2), dtype=torch.float32, device="cuda", generator=g))
        n = rows * cols
        dst = torch.empty_like(x)
        copy_ms = median_ms(lambda: dst.copy_(x), args.iters, torch)
        del dst
        for hop in (2048, 1024):
            sp = pkg.Spectrum(hop=hop)
            spectrum_ms = median_ms(lambda: sp.process_bulk(x.reshape(-1)), args.iters, torch)
            ls = pkg.LineSpectrum(hop=hop)
            for statistic in ("envelope", "square", "fourth"):
                ms = median_ms(lambda: ls.process_rows(x, None, statistic, normalize=False), args.iters, torch)
                print(json.dumps({"tool": "benchmark_line_spectrum", "rows": rows, "cols": cols, "hop": hop,
                                  "statistic": statistic, "ms": round(ms, 4), "gitems_per_s": round(n / ms / 1e6, 2),
                                  "read_tb_per_s": round(8 * n / ms / 1e9, 3), "spectrum_ms": round(spectrum_ms, 4),
                                  "over_spectrum": round(ms / spectrum_ms, 3), "copy_ms": round(copy_ms, 4),
                                  "copy_tb_per_s": round(16 * n / copy_ms / 1e9, 3),
                                  "device": torch.cuda.get_device_name(0)}), flush=True)
        del x


if __name__ == "__main__":
    main()
