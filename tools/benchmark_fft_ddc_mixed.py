#!/usr/bin/env python3
"""Rate of the MixedFftDdc block (csrc/fft_ddc.hip) beside what it replaces, all in the same process.

  tools/benchmark_fft_ddc_mixed.py [--log2-items 28] [--iters 20]

K = 24 channels, 8 each at D = 16, 32 and 64, default taps (12 a phase), two images, over one call of 2^log2-items
wideband samples into a preallocated output, for complex64 and sc16 input; timed with device events, the median over
the iterations:
  mixed      one MixedFftDdc of all 24 channels (its default overlap, 768)
  three      three FftDdc handles of 8 channels each at D = 16, 32, 64 and the same overlap, one after the other: what a
             user does without the block
  all_at_16  FftDdc of the 24 frequencies at D = 16 and the same overlap
Prints one JSON line per format."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchmark_channelizer import median_ms  # noqa: E402

DECIMATIONS = [16] * 8 + [32] * 8 + [64] * 8


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
    K = len(DECIMATIONS)
    freqs = list(np.random.default_rng(K).uniform(-0.5, 0.5, K))
    mixed = pkg.MixedFftDdc(freqs, DECIMATIONS)
    V = mixed.overlap
    three = [pkg.FftDdc(freqs[lo:lo + 8], DECIMATIONS[lo], overlap=V) for lo in (0, 8, 16)]
    at16 = pkg.FftDdc(freqs, 16, overlap=V)
    out = torch.empty((K, n // 16 + 1), dtype=torch.complex64, device="cuda")
    for name, src in (("cf32", x), ("sc16", xi)):
        def run_mixed():
            mixed.reset()
            mixed.process_bulk(src, out=out)

        def run_three():
            for i, h in enumerate(three):
                h.reset()
                h.process_bulk(src, out=out[8 * i:8 * i + 8])

        def run_at16():
            at16.reset()
            at16.process_bulk(src, out=out)

        ms = median_ms(run_mixed, args.iters, torch)
        ms_three = median_ms(run_three, args.iters, torch)
        ms_16 = median_ms(run_at16, args.iters, torch)
        print(json.dumps({"tool": "benchmark_fft_ddc_mixed", "channels": K, "decimations": "8 x 16, 8 x 32, 8 x 64", "overlap": V,
                          "images": 2, "format": name, "items": n, "mixed_ms": round(ms, 4),
                          "mixed_gsamples_per_s": round(n / ms / 1e6, 2), "three_handles_ms": round(ms_three, 4),
                          "three_over_mixed": round(ms_three / ms, 3), "all_at_16_ms": round(ms_16, 4),
                          "all_at_16_over_mixed": round(ms_16 / ms, 3), "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
