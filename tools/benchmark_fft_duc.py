#!/usr/bin/env python3
"""Rate of the FftDuc block (csrc/fft_duc.hip) beside the Duc of the same taps and a copy of the output's bytes, all in the
same process.

  tools/benchmark_fft_duc.py [--log2-items 28] [--iters 20] [--format sc16|sc8|cu8]

One process_bulk() call of 2^log2-items / 16 items per row (2^log2-items output samples from the Duc; the FftDuc delivers
the whole segments among them) into a preallocated output per iteration, timed with device events; the median over the
iterations, in Gsamples/s of output, at K = 8 and K = 64 rows, I = 16 (192 taps, overlap 256, two images).  Beside each:
Duc(the same frequencies, 16, taps=the same) on the same rows, and a device copy of the output's bytes.  Prints one JSON
line per K.  --format F: per K also the integer output (gr4pm_fft_duc_process_iq), three more figures
from the same process (tools/iq_out_timing.py): the fused call that writes F, the complex64 call again, and that call
followed by iq_pack()."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchmark_channelizer import median_ms  # noqa: E402
from iq_out_timing import iq_out_figures  # noqa: E402

I = 16


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2-items", type=int, default=28)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--format", choices=["sc16", "sc8", "cu8"], help="also the integer output: fused, complex64, complex64 + iq_pack")
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    assert torch.cuda.is_available(), "needs a GPU"
    n = 1 << args.log2_items
    items = n // I
    g = torch.Generator(device="cuda").manual_seed(1)
    taps = pkg.fft_duc_taps(I)
    out = torch.empty(n, dtype=torch.complex64, device="cuda")
    other = torch.empty_like(out)
    ms_copy = median_ms(lambda: other.copy_(out), args.iters, torch)
    for K in (8, 64):
        v = torch.view_as_complex(torch.randn((K, items, 2), dtype=torch.float32, device="cuda", generator=g))
        freqs = list(np.random.default_rng(K).uniform(-0.5, 0.5, K))
        fd = pkg.FftDuc(freqs, I, taps=taps)
        duc = pkg.Duc(freqs, I, taps=taps, max_items=items)
        samples = fd.output_items(items)

        def run_fd():
            fd.reset()
            fd.process_bulk(v, out=out)

        def run_duc():
            duc.reset()
            duc.process_bulk(v, out=out)

        ms = median_ms(run_fd, args.iters, torch)
        ms_duc = median_ms(run_duc, args.iters, torch)
        def run_format(**kw):
            fd.reset()
            return fd.process_bulk(v, **kw)

        extra = iq_out_figures(pkg, torch, median_ms, args.iters, args.format, n, run_format) if args.format else {}
        print(json.dumps({"tool": "benchmark_fft_duc", "channels": K, "interpolation": I, "taps": int(taps.size),
                          "overlap": fd.overlap, "images": fd.images, "items_per_row": items, "samples": samples,
                          "ms": round(ms, 4), "gsamples_per_s": round(samples / ms / 1e6, 2), "duc_ms": round(ms_duc, 4),
                          "duc_gsamples_per_s": round(n / ms_duc / 1e6, 2), "over_duc": round(ms_duc / ms, 3),
                          "copy_ms": round(ms_copy, 4), "over_copy": round(ms / ms_copy, 3), **extra,
                          "device": torch.cuda.get_device_name(0)}), flush=True)
        del fd, duc, v


if __name__ == "__main__":
    main()
