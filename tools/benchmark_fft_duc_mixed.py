#!/usr/bin/env python3
"""Rate of the MixedFftDuc block (csrc/fft_duc.hip) beside what it replaces, all in the same process.

  tools/benchmark_fft_duc_mixed.py [--log2-items 28] [--iters 20] [--format sc16|sc8|cu8]

K = 24 rows, 8 each at I = 16, 32 and 64, default taps (12 a phase), two images, over one call of 2^log2-items output
samples' worth of items (2^log2-items / I_k items in row k; the whole segments among them are delivered) into a
preallocated output; timed with device events, the median over the iterations:
  mixed      one MixedFftDuc of all 24 rows (its default overlap, 768)
  three      three FftDuc handles of 8 rows each at I = 16, 32, 64 and the same overlap into three outputs, and the two
             additions that make one stream of them: what a user does without the block
  all_at_16  FftDuc of the 24 frequencies at I = 16 and the same overlap (every row with the I = 16 rows' item count)
Prints one JSON line.  --format F: also the integer output of the mixed handle (gr4pm_fft_duc_mixed_process_iq, DESIGN
section 31), three more figures from the same process (tools/iq_out_timing.py): the fused call that writes F, the
complex64 call again, and that call followed by iq_pack()."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchmark_channelizer import median_ms  # noqa: E402
from iq_out_timing import iq_out_figures  # noqa: E402

INTERPOLATIONS = [16] * 8 + [32] * 8 + [64] * 8


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
    K = len(INTERPOLATIONS)
    g = torch.Generator(device="cuda").manual_seed(1)
    v = torch.view_as_complex(torch.randn((K, n // 16, 2), dtype=torch.float32, device="cuda", generator=g))
    freqs = list(np.random.default_rng(K).uniform(-0.5, 0.5, K))
    mixed = pkg.MixedFftDuc(freqs, INTERPOLATIONS)
    V, slots = mixed.overlap, n // mixed.slot
    three = [pkg.FftDuc(freqs[lo:lo + 8], INTERPOLATIONS[lo], overlap=V) for lo in (0, 8, 16)]
    at16 = pkg.FftDuc(freqs, 16, overlap=V)
    samples = mixed.output_items(slots)
    assert all(h.output_items(n // h.interpolation) == samples for h in three + [at16])
    out = torch.empty(n, dtype=torch.complex64, device="cuda")
    parts = [torch.empty(n, dtype=torch.complex64, device="cuda") for _ in range(2)]

    def run_mixed():
        mixed.reset()
        mixed.process_bulk(v, slots, out=out)

    def run_three():
        for h, lo, o in zip(three, (0, 8, 16), [out] + parts):
            h.reset()
            h.process_bulk(v[lo:lo + 8, :n // h.interpolation], out=o)
        torch.add(out[:samples], parts[0][:samples], out=out[:samples])
        torch.add(out[:samples], parts[1][:samples], out=out[:samples])

    def run_at16():
        at16.reset()
        at16.process_bulk(v, out=out)

    ms = median_ms(run_mixed, args.iters, torch)
    ms_three = median_ms(run_three, args.iters, torch)
    ms_16 = median_ms(run_at16, args.iters, torch)

    def run_format(**kw):
        mixed.reset()
        return mixed.process_bulk(v, slots, **kw)

    extra = iq_out_figures(pkg, torch, median_ms, args.iters, args.format, n, run_format) if args.format else {}
    print(json.dumps({"tool": "benchmark_fft_duc_mixed", "rows": K, "interpolations": "8 x 16, 8 x 32, 8 x 64", "overlap": V, "images": 2,
                      "samples": samples, "mixed_ms": round(ms, 4), "mixed_gsamples_per_s": round(samples / ms / 1e6, 2),
                      "three_handles_ms": round(ms_three, 4), "three_over_mixed": round(ms_three / ms, 3),
                      "all_at_16_ms": round(ms_16, 4), "all_at_16_over_mixed": round(ms_16 / ms, 3), **extra,
                      "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
