#!/usr/bin/env python3
"""Rate of the FftDdc block (csrc/fft_ddc.hip) beside the Ddc of the same taps and the Spectrum of the same hop, all in the
same process.

  tools/benchmark_fft_ddc.py [--log2-items 28] [--iters 20]

One process_bulk() call of 2^log2-items wideband samples into a preallocated output per iteration, timed with device
events; the median over the iterations, in Gsamples/s of input, at K = 8 and K = 64 channels, D = 16 (192 taps, overlap
256, two images), for complex64 and sc16 input.  Beside each: Ddc(the same frequencies, 16, taps=the same) on the same
stream, and Spectrum(hop = 2048 - overlap), the cost of the shared forward transform alone.  Prints one JSON line per
(K, format)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchmark_channelizer import median_ms  # noqa: E402

D = 16


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2-items", type=int, default=28)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    assert torch.cuda.is_available(), "needs a GPU"
    n = 1 << args.log2_items
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.randn((n, 2), dtype=torch.float32, device="cuda", generator=g))
    xi = pkg.iq_pack(x, "sc16", 0.125 * 32768.0)
    taps = pkg.fft_ddc_taps(D)
    for K in (8, 64):
        freqs = list(np.random.default_rng(K).uniform(-0.5, 0.5, K))
        fd = pkg.FftDdc(freqs, D, taps=taps)
        ddc = pkg.Ddc(freqs, D, taps=taps, max_frames=n // D + 1)
        sp = pkg.Spectrum(hop=fd.hop)
        out = torch.empty((K, n // D + 1), dtype=torch.complex64, device="cuda")
        for name, src in (("cf32", x), ("sc16", xi)):
            def run_fd():
                fd.reset()
                fd.process_bulk(src, out=out)
            def run_ddc():
                ddc.reset()
                ddc.process_bulk(src, out=out)
            ms = median_ms(run_fd, args.iters, torch)
            ms_ddc = median_ms(run_ddc, args.iters, torch)
            ms_sp = median_ms(lambda: sp.process_bulk(src), args.iters, torch)
            print(json.dumps({"tool": "benchmark_fft_ddc", "channels": K, "decimation": D, "taps": int(taps.size),
                              "overlap": fd.overlap, "images": fd.images, "format": name, "items": n, "ms": round(ms, 4),
                              "gsamples_per_s": round(n / ms / 1e6, 2), "ddc_ms": round(ms_ddc, 4),
                              "ddc_gsamples_per_s": round(n / ms_ddc / 1e6, 2), "over_ddc": round(ms_ddc / ms, 3),
                              "spectrum_ms": round(ms_sp, 4), "over_spectrum": round(ms / ms_sp, 3),
                              "device": torch.cuda.get_device_name(0)}), flush=True)
        sp.read()
        del fd, ddc, sp, out


if __name__ == "__main__":
    main()
