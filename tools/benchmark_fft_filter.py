#!/usr/bin/env python3
"""Rate of the FftFilter block (csrc/fft_filter.hip) against a copy of the bytes it moves and the one-bin correlator, all
in the same process.

  tools/benchmark_fft_filter.py [--log2-items 28] [--iters 20]

One process_bulk() call of 2^log2-items wideband samples per iteration into a caller's buffer, timed with device events;
the median over the iterations, for an overlap of 256 (257 taps) and of 1024 (1025 taps) and for complex64 and sc16
input.  Beside each: torch's device-to-device copy of as many bytes as the filter reads and writes (8 or 4 read, 8
written per sample), and SyncwordDetection.correlate_only with one frequency bin on complex64 samples: the same two
transforms and one product per block of 1752 samples, storing powers (half the bytes) where the filter stores samples.
Prints one JSON line per (overlap, format) with Gsamples/s, TB/s read plus written, and the time per segment beside the
correlator's time per block."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchmark_channelizer import median_ms  # noqa: E402

CORRELATOR_BLOCK = 1752  # the correlator's stride: new samples per overlap-save block of 2048


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2-items", type=int, default=28)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as ge
    import bench
    pkg = ge.load_package()
    assert torch.cuda.is_available(), "needs a GPU"
    n = 1 << args.log2_items
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.randn((n, 2), dtype=torch.float32, device="cuda", generator=g))
    xi = pkg.iq_pack(x, "sc16", 0.125 * 32768.0)
    out = torch.empty(n, dtype=torch.complex64, device="cuda")
    rrc = bench.unit_norm_rrc(pkg)
    sd = pkg.SyncwordDetection(rrc, bench.SYNCWORD, np.array([1, -1], dtype=np.complex64), 0, 0, power_threshold=9.5, max_items=n)
    ms_corr = median_ms(lambda: sd.correlate_only(x), args.iters, torch)
    us_block = 1e3 * ms_corr / (n / CORRELATOR_BLOCK)
    copies = {}
    for name, item_bytes in (("cf32", 8), ("sc16", 4)):
        half = (item_bytes + 8) * n // 2  # a copy reads and writes this many bytes each
        src = torch.empty(half, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        copies[name] = median_ms(lambda: dst.copy_(src), args.iters, torch)
        del src, dst
    rng = np.random.default_rng(3)
    for overlap in (256, 1024):
        taps = (rng.standard_normal(overlap + 1) + 1j * rng.standard_normal(overlap + 1)).astype(np.complex64)
        f = pkg.FftFilter(taps / np.sqrt(overlap + 1), overlap=overlap)
        for name, src, item_bytes in (("cf32", x, 8), ("sc16", xi, 4)):
            def call():
                f.reset()
                f.process_bulk(src, out=out)
            ms = median_ms(call, args.iters, torch)
            segments = n // f.hop
            gsps = n / ms / 1e6
            us_segment = 1e3 * ms / segments
            print(json.dumps({"tool": "benchmark_fft_filter", "overlap": overlap, "hop": f.hop, "format": name, "items": n,
                              "ms": round(ms, 4), "gsamples_per_s": round(gsps, 2),
                              "tb_per_s": round((item_bytes + 8) * gsps / 1e3, 3), "segments": segments,
                              "ns_per_segment": round(1e3 * us_segment, 2),
                              "copy_ms": round(copies[name], 4), "copy_tb_per_s": round((item_bytes + 8) * n / copies[name] / 1e9, 3),
                              "one_bin_correlator_ms": round(ms_corr, 4),
                              "one_bin_correlator_gsamples_per_s": round(n / ms_corr / 1e6, 2),
                              "one_bin_correlator_ns_per_block": round(1e3 * us_block, 2),
                              "segment_over_block": round(us_segment / us_block, 3), "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
